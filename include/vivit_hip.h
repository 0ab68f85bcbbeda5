/*
 * vivit_hip.h -- C ABI of libvivit_hip.so, the MI355X (gfx950) kernel library behind the
 * low-rank GGN curvature path of ViViT (Gram build V^T V  +  symmetric eigendecomposition
 * + Gram-space -> parameter-space maps).
 *
 * The reference (f-dangel/vivit) is pure Python and has no FFI; each entry point below names
 * the reference call site (path:line under /root/reference) whose tensor op it replaces.  A
 * Python maintainer binds these with ctypes; nothing here uses torch
 * types.
 *
 * Conventions (all entry points):
 *   - every pointer is a DEVICE pointer to fp32 row-major data owned by the caller, unless the
 *     parameter is documented as a host pointer; leading dimensions are in ELEMENTS;
 *   - `stream` is a hipStream_t passed as void* (NULL = the default stream); calls only enqueue
 *     work and never synchronise, allocate or free device memory; scratch memory comes from the
 *     caller through (workspace, workspace_bytes) sized by the matching *_workspace_bytes query;
 *   - return value: 0 = ok; <0 = bad argument (VIVIT_E_*); a numerical failure of the
 *     eigensolver is reported asynchronously through the device-side `info` word
 *     (0 = converged, k>0 = k off-diagonal elements did not converge; n = non-finite input), which the host maps
 *     to the reference's RuntimeError (vivit/utils/eig.py:37-40,103-106).  VIVIT_INFO_PERSIST_TIMEOUT (< 0) is a
 *     failure of a different kind -- see "Persistent kernels" below;
 *   - results are deterministic (bit-identical from call to call and from process to process on the same device
 *     type; tests/test_determinism_gpu.py): every reduction has a fixed order.  The one kernel that uses float
 *     atomics, the bf16-pipe 256 x 256 tile product, adds the partial sum of each 4096-k accumulation chain into C
 *     with no-return fp32 atomics executed at the memory side -- each output element has exactly ONE writing
 *     workgroup and ONE writing lane, whose adds to that address are issued and applied in program order, so the
 *     sum is a fixed-order sum; no two workgroups ever add into the same element.
 */
#ifndef VIVIT_HIP_H
#define VIVIT_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define VIVIT_OK 0
#define VIVIT_E_BADARG (-1)     /* null pointer, negative size, ld too small               */
#define VIVIT_E_WORKSPACE (-2)  /* workspace missing or smaller than *_workspace_bytes      */
#define VIVIT_E_LAUNCH (-3)     /* hipLaunch reported an error (hipGetLastError != success) */
#define VIVIT_E_UNSUPPORTED (-4)

/* ---------------------------------------------------------------------------------------------
 * Persistent kernels.  Three stages of the eigensolver run as ONE launch whose workgroups exchange data through the
 * L2 and therefore must all be resident at once: the tridiagonalisation for n <= 2048 (sytrd_persist.hip), the panel QR
 * of the band reduction (sy2sb.hip) and the bulge chase (sb2st.hip).  Whether they are is decided once per launch by an
 * atomic arrival gate BEFORE anything is written; a launch that does not become resident within 2 s (another process or
 * a long-running kernel of another stream holds its compute units) aborts untouched and ONE retry queued behind it
 * runs.  If that fails too -- or an exchange stalls later -- the stage gives up, the solve's `info` word becomes
 * VIVIT_INFO_PERSIST_TIMEOUT (its results are garbage) and the library stays usable.  This status is distinct from the
 * numerical ones: the input may be perfectly fine.  The host wrapper (vivit_amd/kernels.py) raises
 * PersistentKernelTimeout and, when it still holds the input, repeats the solve ONCE with vivit_persistent_kernels(0),
 * i.e. on the launch chains (VIVIT_SYTRD_PERSIST / VIVIT_QR_PERSIST / VIVIT_SB2ST_PERSIST = 0 select them for good).
 * ------------------------------------------------------------------------------------------- */
#define VIVIT_INFO_PERSIST_TIMEOUT (-1000)
/* 1 / 0: allow / forbid the persistent kernels for the following calls of this process (overrides the environment
 * variables); -1: back to the environment's choice.  Returns the previous setting (-1, 0 or 1).  Host-side state only. */
int vivit_persistent_kernels(int on);
/* For callers of the STAGE-level entry points (vivit_sytrd_f32, vivit_sy2sb_f32, vivit_sy2sb_panel_qr_f32,
 * vivit_sb2st_f32), which have no info word: *info (device) = VIVIT_INFO_PERSIST_TIMEOUT if a persistent kernel launched on
 * `stream` gave up since that stream's failure word was last taken, and clears the word (there is one word per device and
 * stream, so a solve on another stream is never blamed); *info is left alone otherwise.  The vivit_symeig*_f32 entry
 * points do this themselves.  (A stage that gave up also poisons its output with NaN, so nothing fails silently.) */
int vivit_take_persist_timeout(int32_t *info, void *stream);

/* Library/ABI version (major*1000 + minor) and the gfx target it was compiled for. */
int vivit_hip_abi_version(void);   /* 1008 in this release; _lib.py refuses any other library */
const char *vivit_hip_target(void);
/* Provenance: the content hash (32 hex digits, vivit_amd/_build.py:source_hash) of the csrc/ tree + this header the library
 * was compiled from ("unknown" for a build that did not go through _build.py).  _lib.load() compares it with the sources
 * beside the package and refuses a stale binary. */
const char *vivit_hip_source_hash(void);
const char *vivit_hip_status_string(int status);

/* ---------------------------------------------------------------------------------------------
 * K1  Gram contraction (SYRK):  G = alpha * A A^T + beta * G
 *   A: [n, p] (one parameter's V_t viewed as [C*N, P_param]; K-contiguous rows, lda >= p)
 *   G: [n, n] full symmetric output (both triangles written), ldg >= n.
 * Replaces partial_contract(V, V, (2, 2)) = einsum("cn<p>,dm<p>->cndm")
 *   vivit/utils/gram.py:206-232 via pairwise_dot :9-35; callers
 *   vivit/extensions/secondorder/vivit/base.py:118-124,
 *   vivit/extensions/secondorder/sqrt_ggn/gram_sqrt_ggn.py:50-52,
 *   vivit/optim/directional_damped_newton.py:254, and the `gram += gram_p` accumulation of
 *   vivit/utils/gram.py:104-116 (beta = 1).
 * Only the lower-triangular tiles (256x256 for large outputs with a long contraction, 128x128 otherwise) are
 * computed on MFMA (n(n+1)p flops); the mirror tiles are transposed through LDS and stored as well.
 * ------------------------------------------------------------------------------------------- */
/* Matrix pipe of the large K-contiguous products (the Gram SYRK above a few hundred 256 x 256 tiles and K >= 1024, the NT
 * GEMMs of the same size, and Gram matrices of small batches with a deep contraction): 6 (default) = bf16 MFMA pipe --
 * every fp32 operand is split EXACTLY into three bf16 pieces (a = hi + mid + lo, 24 significand bits) and a product is
 * the sum of the six partial products that are >= 2^-16 of it, each exact in the MFMA, accumulated in fp32 (the three
 * dropped ones are < 2^-24 |a b|, below the rounding of an fp32 product); 9 = all nine partial products; 3 = three
 * (per-product error 2^-16: exists so that tests can show they would notice); 0 = v_mfma_f32_32x32x2_f32 on the fp32
 * operands.  Set once per process by the environment variable VIVIT_GEMM_SPLIT.  The split pieces of a 65 536-column
 * chunk live in the workspace (6 bytes per element of the chunk).
 *
 * INPUT RANGE CONTRACT (tests/test_gram_precision_gpu.py).  The split is exact only for finite values whose smallest
 * piece is a normal bf16 number.  The split pass therefore flags, per column chunk, (bit 0) any value that is +-inf,
 * NaN or rounds to +-inf as bf16 (|a| >= 3.3962e38) and (bit 1) any non-zero value below 2^-100; the bf16-pipe launch
 * of a flagged chunk returns at once and the fp32 MFMA kernel, always launched behind it on the same columns (and
 * returning at once for an unflagged chunk -- there is no host synchronisation), computes that chunk instead.  Every
 * entry point in this header thus has the semantics of a k-ordered fp32 fma chain for EVERY input: inf/NaN propagate
 * as in IEEE fp32, 3.4e38 * 0.5 is finite, denormal inputs are multiplied as fp32 denormals.  The 64-row streaming
 * product (outputs of at most 64 rows, N and K >= 2048) gathers the same two bits over both whole operands while it
 * splits them, always writes its split-K slab, and the fp32 MFMA kernel behind it on the same grid rewrites the slab
 * when a bit is set; its bf16 form is used only while every lane's byte offset into B fits in 32 bits (K-contiguous
 * B: ldb <= 4 210 751 floats; k-major B: ldb <= 71 582 771), wider operands take the fp32 kernel
 * (tests/test_gemm_contract_gpu.py checks every route).  Internal products of the eigensolver on the 256-tile and
 * split-K routes honour bit 0 only; the band reduction's internal 64-row product does not gate at all. */
int vivit_gemm_split_mode(void);
size_t vivit_gram_syrk_f32_workspace_bytes(int64_t n, int64_t p);
int vivit_gram_syrk_f32(const float *A, int64_t n, int64_t p, int64_t lda, float *G, int64_t ldg,
                        float alpha, float beta, void *workspace, size_t workspace_bytes,
                        void *stream);

/* ---------------------------------------------------------------------------------------------
 * K2/K5/K9  C = alpha * A B^T + beta * C      A: [m, k] lda, B: [n, k] ldb, C: [m, n] ldc
 * Replaces partial_contract(V, g, (2, 1))  vivit/optim/directional_damped_newton.py:255,
 *   mVp  vivit/utils/gram.py:182-203, and the gamma einsum "in,id->nd" (on transposed views)
 *   vivit/optim/directional_damped_newton.py:342.
 * ------------------------------------------------------------------------------------------- */
size_t vivit_gemm_f32_workspace_bytes(int64_t m, int64_t n, int64_t k);
int vivit_gemm_nt_f32(const float *A, const float *B, float *C, int64_t m, int64_t n, int64_t k,
                      int64_t lda, int64_t ldb, int64_t ldc, float alpha, float beta,
                      void *workspace, size_t workspace_bytes, void *stream);

/* K6/K7/K8  C = alpha * A B + beta * C        A: [m, k] lda, B: [k, n] ldb, C: [m, n] ldc
 * Replaces Vmp  vivit/utils/ggn.py:94-115 (eigenvector back-projection, eigh.py:267-270),
 *   the Newton-step back-projection einsum("cn,cn...->...")
 *   vivit/optim/directional_damped_newton.py:370-373 (m = 1), and "cni,id->cnd" :348-350. */
int vivit_gemm_nn_f32(const float *A, const float *B, float *C, int64_t m, int64_t n, int64_t k,
                      int64_t lda, int64_t ldb, int64_t ldc, float alpha, float beta,
                      void *workspace, size_t workspace_bytes, void *stream);

/* C = alpha * A^T B + beta * C                A: [k, m] lda, B: [k, n] ldb, C: [m, n] ldc
 * Replaces einsum("in,id->nd")  vivit/optim/directional_damped_newton.py:342 without a
 * transposed copy, and Y^T Z in the Householder back-transformation of the eigensolver. */
int vivit_gemm_tn_f32(const float *A, const float *B, float *C, int64_t m, int64_t n, int64_t k,
                      int64_t lda, int64_t ldb, int64_t ldc, float alpha, float beta,
                      void *workspace, size_t workspace_bytes, void *stream);

/* ---------------------------------------------------------------------------------------------
 * K1'  Factorised Gram of a Linear weight:  G[c,n,d,m] = alpha * Gz[n,m] * Gs[c,n,d,m] + beta*G
 *   Gz: [N, N] (z z^T), Gs: [C*N, C*N] (s s^T), G: [C*N, C*N], all contiguous.
 * Replaces einsum("nm,cndm->cndm")  vivit/extensions/secondorder/vivit/linear.py:72-75.
 * ------------------------------------------------------------------------------------------- */
int vivit_gram_hadamard_f32(const float *Gz, const float *Gs, float *G, int64_t C, int64_t N,
                            float alpha, float beta, void *stream);

/* Rectangular block of the same product: rows (c, n) with c < Cr, n < Nr; columns (d, m) with d < Cc, m < Nc:
 *   G[(c,n), (d,m)] = alpha * Gz[n, m] * Gs[(c,n), (d,m)] + beta * G[(c,n), (d,m)]
 *   Gz: [Nr, Nc], Gs: [Cr*Nr, Cc*Nc] contiguous; G: [Cr*Nr, Cc*Nc] with leading dimension ldg.
 * Used for (i) the block row G[N_g, :] of a batch shard in the data-parallel Gram build (Nr = local samples,
 * Nc = all samples; the reference has no multi-device code: SURVEY.md 8e) and (ii) V^T g of a factorised Linear
 * weight, einsum("cno,ni,mo,mi->cnm"): the factorised form of partial_contract(V, g, (2, 1))
 * vivit/optim/directional_damped_newton.py:255 with V as in linear.py:41-42 (Cc = 1). */
int vivit_gram_hadamard_block_f32(const float *Gz, const float *Gs, float *G, int64_t Cr, int64_t Nr, int64_t Cc,
                                  int64_t Nc, int64_t ldg, float alpha, float beta, void *stream);

/* ---------------------------------------------------------------------------------------------
 * Factorised Gram of a Linear weight on a sequence input [N, T, in] (any extra dimensions between batch and features,
 * vivit/extensions/secondorder/vivit/linear.py:38-39, flattened into T): with s = [C, N, T, O] the factor at the module output and
 * z = [N, T, I] the input, V_t[c,n,o,i] = sum_t s[c,n,t,o] z[n,t,i] and
 *   G[(c,n), (e,m)] = sum_{t,u < T} Gs[(c,n,t), (e,m,u)] * Gz[(n,t), (m,u)],   Gs = s' s'^T (s' = [C N T, O]), Gz = z' z'^T (z' = [N T, I]).
 * vivit_gram_seq_reduce_f32 is the last step, on a rectangular block (rows (c, n) with c < Cr, n < Nr; columns (e, m), e < Cc, m < Nc):
 *   G[(c Nr + n) ldg + e Nc + m] = alpha * sum_{t<T} sum_{u<T} Gz[(n T + t) ldz + m T + u] * Gs[((c Nr + n) T + t) lds + (e Nc + m) T + u]
 *                                  + beta * G[...]                 (G is not read when beta == 0)
 *   Gz: [Nr T, >= Nc T] ldz, Gs: [Cr Nr T, >= Cc Nc T] lds, G: [Cr Nr, >= Cc Nc] ldg; columns of G beyond Cc Nc are left untouched.
 * Call site: the row slabs of route A of vivit_amd/backend/extensions.py:_linear_seq_weight_closures (ViViTGGN{Exact,MC}).
 * No atomics.  The summation order of an entry depends on T alone (per u an fma chain over t, then the T sums added in the order
 * of u, then alpha, then fma(beta, G, .)): the bytes of an entry are a function of its two T x T operand blocks, alpha, beta and
 * the prior entry, whatever its position, the block's sizes or the operands' alignment.  T = 1 gives the bytes of
 * vivit_gram_hadamard_block_f32.  Operands 16-byte aligned with ldz, lds and Nc T multiples of 4 take the float4 body.
 * Status: negative sizes, ldz < Nc T, lds < Cc Nc T, ldg < Cc Nc, or a null pointer with non-zero sizes: VIVIT_E_BADARG; any zero
 * size: VIVIT_OK, nothing is launched.  LIMITS (VIVIT_E_UNSUPPORTED beyond them): T <= 1024 (a T x T block is summed by one
 * workgroup); every size, leading dimension, Cr Nr T and Cc Nc T below 2^31; for T > 1 at most 2^24 - 1 rows Cr Nr (one
 * workgroup of 256 lanes per row along the grid's first dimension) and at most 65 535 column spans of (1024 / T rounded down to a
 * multiple of 4 / gcd(T, 4)) outputs.
 * ------------------------------------------------------------------------------------------- */
int vivit_gram_seq_reduce_f32(const float *Gz, int64_t ldz, const float *Gs, int64_t lds, float *G, int64_t ldg,
                              int64_t Cr, int64_t Nr, int64_t Cc, int64_t Nc, int64_t T,
                              float alpha, float beta, void *stream);

/* Length-C contractions of the factorised Linear products (the MFMA GEMM with z does the rest):
 *   vivit_class_contract_f32:  T[f, o, n] = sum_c mat[f, c, n] * s[c, n, o]      mat: [F,C,N], s: [C,N,O], T: [F,O,N]
 *     first half of einsum("cno,vcn,ni->voi")  vivit/extensions/secondorder/vivit/linear.py:53
 *   vivit_class_expand_f32:    R[f, c, n] = sum_o s[c, n, o] * U[f, o, n]        U: [F,O,N], R: [F,C,N]
 *     second half of einsum("cno,voi,ni->vcn")  vivit/extensions/secondorder/vivit/linear.py:64 */
int vivit_class_contract_f32(const float *mat, const float *s, float *T, int64_t F, int64_t C, int64_t N, int64_t O,
                             void *stream);
int vivit_class_expand_f32(const float *s, const float *U, float *R, int64_t F, int64_t C, int64_t N, int64_t O,
                           void *stream);

/* ---------------------------------------------------------------------------------------------
 * Factor materialisation (f1): per-sample parameter Jacobian-transpose products, the `param_mjp(..., sum_batch=False)`
 * call of vivit/extensions/secondorder/vivit/base.py:84-92 (BackPACK LinearDerivatives / Conv2DDerivatives).
 *   vivit_linear_weight_mjp_f32: V[(c,n), o, i] = s[(c,n), o] * z[n, i]       s: [C*N, O], z: [N, I], V: [C*N, O*I]
 *     (einsum "vno,ni->vnoi"; what linear.py:41-42 keeps factorised, materialised for SqrtGGN{Exact,MC} / BatchGrad)
 *   vivit_conv2d_weight_mjp_f32: V[r, o, c, kh, kw] = sum_{oh,ow} M[r, o, oh, ow] * x[r % N, c, oh*sh-ph+kh*dh, ow*sw-pw+kw*dw]
 *     M: [rows, Cout, OH, OW], x: [N, Cin, H, W], V: [rows, Cout*Cin*KH*KW]; rows = C*N (class-major), groups = 1,
 *     zero padding (unfold + einsum "vnol,nkl->vnok" without the im2col buffer).  Per row a GEMM on the fp32 matrix pipe
 *     when the sample's zero-bordered planes and the row of M fit the LDS (and OW >= 4), else a scalar kernel; the two
 *     differ in summation order only (VIVIT_CONV_MFMA=0 selects the scalar kernels).
 * The Linear rule is bound by the 4*rows*P bytes it writes.
 * ------------------------------------------------------------------------------------------- */
int vivit_linear_weight_mjp_f32(const float *s, const float *z, float *V, int64_t C, int64_t N, int64_t O, int64_t I,
                                void *stream);
int vivit_conv2d_weight_mjp_f32(const float *M, const float *x, float *V, int64_t rows, int64_t N, int64_t Cin, int64_t H,
                                int64_t W, int64_t Cout, int64_t KH, int64_t KW, int64_t OH, int64_t OW, int64_t sh,
                                int64_t sw, int64_t ph, int64_t pw, int64_t dh, int64_t dw, void *stream);

/* ---------------------------------------------------------------------------------------------
 * f1  Back-propagation of the sqrt-GGN factor through the layers (jacobians.hip): the transposed input-Jacobian products
 *   M [V, N, *out] -> [V, N, *in]  that BackPACK's derivative classes supply to the reference through `MatToJacMat`
 *   (vivit/extensions/secondorder/vivit/__init__.py:84-118, base.py:19,41), the loss-Hessian square roots that seed it
 *   (SqrtGGNCrossEntropyLoss, __init__.py:84-86) and the reductions of the bias / BatchNorm parameter rules
 *   (base.py:84-92 -> param_mjp).  All tensors contiguous fp32, `V` slices outermost.
 * ------------------------------------------------------------------------------------------- */
/* out[v, e] = M[v, e] * f'(x[e]), e < per_v (= N * features).  kind: 0 ReLU, 1 Sigmoid, 2 Tanh, 3 LeakyReLU (param =
 * negative slope), 4 LogSigmoid, 5 ELU (param = alpha), 6 SELU, 7 GELU (erf form: Phi(x) + x phi(x)), 8 GELU (tanh
 * approximation, nn.GELU(approximate='tanh')), 9 SiLU (s (1 + x (1 - s)), s = sigmoid(x)), 10 soft cap (f = param tanh(x / param),
 * f' = 1 - tanh^2(x / param); param = the cap, which must be finite and > 0: VIVIT_E_BADARG otherwise; Gemma-2's final logits).  Replaces SqrtGGN{ReLU,Sigmoid,Tanh,
 * LeakyReLU,LogSigmoid,ELU,SELU} (__init__.py:87-93); 7 .. 10 have no counterpart in the reference.  A NaN in x: as torch's
 * autograd of the module -- ReLU passes the factor unchanged and LeakyReLU scales it by the slope (the branch a failed
 * comparison selects there), every other rule gives NaN.  GELU and SiLU at x = +-inf give NaN (the inf * 0 of torch's backward
 * formulas, which are evaluated term by term here), at large finite |x| exactly 1 or (+-)0: no deliberate difference from
 * torch. */
int vivit_act_jac_t_f32(const float *M, const float *x, float *out, int64_t V, int64_t per_v, int kind, float param,
                        void *stream);
/* out[r, c, l] = M[r, c, l] * scale[c]: BatchNorm in eval mode, scale = weight / sqrt(running_var + eps)
 * (vivit/extensions/secondorder/vivit/batchnormnd.py:8-13 -> BatchNormNdDerivatives). */
int vivit_channel_scale_f32(const float *M, const float *scale, float *out, int64_t rows, int64_t C, int64_t L, void *stream);
/* MaxPool2d / AvgPool2d (SqrtGGNMaxPool2d / SqrtGGNAvgPool2d, __init__.py:97-102): planes = N * C of the layer input
 * x [planes, H, W]; M [V * planes, OH, OW] -> out [V * planes, H, W].  idx_ws: planes * OH * OW ints of scratch (the
 * arg-max of every window: first maximum in scan order, as torch).  No ceil_mode, no dilation; average pooling counts
 * the padding (count_include_pad). */
int vivit_maxpool2d_jac_t_f32(const float *M, const float *x, float *out, int *idx_ws, int64_t V, int64_t planes, int64_t H,
                              int64_t W, int64_t OH, int64_t OW, int64_t kh, int64_t kw, int64_t sh, int64_t sw, int64_t ph,
                              int64_t pw, void *stream);
int vivit_avgpool2d_jac_t_f32(const float *M, float *out, int64_t rows_planes, int64_t H, int64_t W, int64_t OH, int64_t OW,
                              int64_t kh, int64_t kw, int64_t sh, int64_t sw, int64_t ph, int64_t pw, void *stream);
/* Conv2d (groups = 1, zero padding): out[r, ci, h, w] = sum_{co, a, b} M[r, co, oh, ow] weight[co, ci, a, b] with
 * oh sh - ph + a dh = h, ow sw - pw + b dw = w  (the transposed convolution; base.py:19 with Conv2DDerivatives,
 * convnd.py:17-22).  rows = V * N.  Filter slices of up to Cout*KH*KW = 1024 run on a scalar kernel (16 input channels per
 * thread, the slice in LDS), larger ones as a per-row GEMM on the fp32 matrix pipe (output channels in chunks that fit the
 * LDS next to the zero-inserted planes of M); VIVIT_E_UNSUPPORTED when neither applies. */
int vivit_conv2d_jac_t_f32(const float *M, const float *weight, float *out, int64_t rows, int64_t Cin, int64_t H, int64_t W,
                           int64_t Cout, int64_t KH, int64_t KW, int64_t OH, int64_t OW, int64_t sh, int64_t sw, int64_t ph,
                           int64_t pw, int64_t dh, int64_t dw, void *stream);
/* out[r] = sum_l M[r, l] * (X ? X[r % rows_x, l] : 1): bias rules (sum over the spatial positions) and the BatchNorm
 * weight rule (X = normalised input of the rows_x = N * C planes, shared by the V slices). */
int vivit_row_dot_f32(const float *M, const float *X, float *out, int64_t rows, int64_t rows_x, int64_t L, void *stream);
/* BatchNorm in eval mode: every rule of the module in ONE pass over the incoming factor M [rows = V N C, L] (L = spatial
 * positions; X [rows_x = N C, L] the module's input): mx[r] = sum_l M[r, l] X[r % rows_x, l] and msum[r] = sum_l M[r, l]
 * (the weight rule sum_l M xhat = (mx - mean_c msum) rstd_c and the bias rule; batchnormnd.py:3 with
 * BatchNormNdDerivatives.param_mjp), out[r, l] = M[r, l] scale[r % C] (the input rule, scale = weight_c rstd_c).  Any of
 * out / mx / msum may be NULL.  Same summation order as vivit_row_dot_f32 (bit-identical sums whenever both take the same
 * body: this kernel takes the 16-byte one when L % 4 == 0 and M, X and out are all 16-byte aligned, vivit_row_dot_f32 looks
 * only at the operands it reads).  wmean / wrstd ([C], both or
 * neither): mx then holds the finished weight rule (mx - wmean_c msum) wrstd_c with wmean = running_mean, wrstd = 1/sqrt(var + eps). */
int vivit_bn_eval_rules_f32(const float *M, const float *X, const float *scale, float *out, float *mx, float *msum, int64_t rows,
                            int64_t rows_x, int64_t C, int64_t L, const float *wmean, const float *wrstd, void *stream);
/* LayerNorm and GroupNorm (norm_rules.hip; no counterpart in the reference's module map).  A normalisation ROW is the set of L
 * contiguous elements that share one mean and variance: nn.LayerNorm on [N, *extra, *D] has rows = N A (A = prod(extra)), L =
 * prod(D); nn.GroupNorm(G, C) on [N, C, *spatial] has rows = N G, L = (C / G) S, S = prod(spatial).  Per row xhat = (x - mean) rstd,
 * h = gamma o M (gamma = 1 when NULL); the index of gamma at position l of a row is (row % G) (L / S) + l / S (LayerNorm: G = S =
 * 1).  All three launches: contiguous fp32, no atomics, fixed summation order; the bytes of a row's results depend on L, S and on
 * the body only -- the 16-byte body is taken when L % 4 == 0 and every operand is 16-byte aligned, a scalar one otherwise.  Rows of
 * L <= 1024 are held in the registers of one wavefront, longer ones by one workgroup. */
/* mean[r] = sum_l X[r, l] / L,  rstd[r] = 1 / sqrt(sum_l (X[r, l] - mean[r])^2 / L + eps)  for X [rows, L]: two passes (never
 * E[x^2] - mean^2).  The statistics nn.LayerNorm / nn.GroupNorm compute in their forward pass. */
int vivit_norm_stats_f32(const float *X, float *mean, float *rstd, int64_t rows, int64_t L, float eps, void *stream);
/* M [V rows, L], X [rows, L], mean / rstd [rows], gamma [G L / S] or NULL.  In one visit of each row:
 *   out[r, l]   = rstd (h - mean_l(h) - xhat mean_l(h xhat))      the transposed input Jacobian of nn.LayerNorm / nn.GroupNorm
 *   seg_w[r, j] = sum_{s < S} M[r, j S + s] xhat[j S + s]         j < L / S
 *   seg_b[r, j] = sum_{s < S} M[r, j S + s]
 * Any of out / seg_w / seg_b may be NULL (not all).  For GroupNorm seg_w / seg_b [V, N, C] are the finished weight and bias rules;
 * for LayerNorm without extra dimensions (S = 1) they are the finished rules M xhat and M.  rows % G == 0, L % S == 0. */
int vivit_norm_rules_f32(const float *M, const float *X, const float *gamma, const float *mean, const float *rstd, float *out,
                         float *seg_w, float *seg_b, int64_t V, int64_t rows, int64_t L, int64_t G, int64_t S, void *stream);
/* nn.LayerNorm with A > 1 positions per sample, M [V, N, A, D], X [N, A, D], mean / rstd [N A]:
 *   pw[v, n, d] = sum_a M[v, n, a, d] (X[n, a, d] - mean[n, a]) rstd[n, a]   (weight rule),   pb[v, n, d] = sum_a M[v, n, a, d]   (bias rule)
 * summed serially over a, one thread per d.  pw or pb may be NULL. */
int vivit_norm_position_sums_f32(const float *M, const float *X, const float *mean, const float *rstd, float *pw, float *pb, int64_t V,
                                 int64_t N, int64_t A, int64_t D, void *stream);
/* nn.RMSNorm, the gated product and rotary position embeddings (llama_rules.hip; no counterpart in the reference's module map): the
 * modules of a LLaMA-style decoder block.  All contiguous fp32, no atomics, fixed summation order.  Status: negative or inconsistent
 * sizes and a NULL pointer with non-zero sizes give VIVIT_E_BADARG, any zero size VIVIT_OK without a launch, sizes beyond the 32-bit
 * index arithmetic or the grid VIVIT_E_UNSUPPORTED.  Every kernel has a 16-byte body (lengths multiples of 4 and every operand
 * 16-byte aligned) and a scalar one.
 * RMSNorm: a ROW is the set of L = prod(normalized_shape) contiguous elements that share one statistic, rows = numel / L, A = rows / N
 * rows per sample.  Rows of L <= 1024 are held in the registers of one wavefront, longer ones by one workgroup, as in norm_rules.hip:
 * the bytes of a row's results depend on L and on the body only. */
/* rstd[r] = 1 / sqrt(sum_l X[r, l]^2 / L + eps)  for X [rows, L]. */
int vivit_rms_norm_stats_f32(const float *X, float *rstd, int64_t rows, int64_t L, float eps, void *stream);
/* M [V rows, L], X [rows, L], rstd [rows], gamma [L] or NULL (= 1).  xhat = x rstd, h = gamma o M; in one visit of each row:
 *   out[v, r, l] = rstd[r] (h - xhat mean_l(h o xhat))      the transposed input Jacobian of nn.RMSNorm
 *   w[v, r, l]   = M[v, r, l] xhat[r, l]                    the weight rule when A == 1
 * out or w may be NULL; both NULL: VIVIT_E_BADARG. */
int vivit_rms_norm_rules_f32(const float *M, const float *X, const float *gamma, const float *rstd, float *out, float *w, int64_t V,
                             int64_t rows, int64_t L, void *stream);
/* nn.RMSNorm with A > 1 rows per sample, M [V, N, A, D], X [N, A, D], rstd [N A]:
 *   pw[v, n, d] = sum_a M[v, n, a, d] X[n, a, d] rstd[n A + a]   (weight rule), summed serially over a, one thread per d. */
int vivit_rms_norm_position_sums_f32(const float *M, const float *X, const float *rstd, float *pw, int64_t V, int64_t N, int64_t A,
                                     int64_t D, void *stream);
/* The product a o b of two branches (vivit_amd.backend.ProductModule; SwiGLU): M [V, n], a / b [n],
 *   Ga[v, i] = M[v, i] b[i]   (the factor handed to a),   Gb[v, i] = M[v, i] a[i]   (the factor handed to b)
 * from one read of M; each result is a single rounded product.  Ga or Gb may be NULL (not both); the operand of a NULL output (a
 * for Gb, b for Ga) is not read and may be NULL. */
int vivit_gate_jac_t_f32(const float *M, const float *a, const float *b, float *Ga, float *Gb, int64_t V, int64_t n, void *stream);
/* Rotary position embedding on the packed projection of the attention module (vivit_amd.backend.RotaryEmbedding; half-split
 * pairing): M, G [R, T, 3, H, d] (R = V N), cosT / sinT [T, d / 2]; d odd: VIVIT_E_BADARG.  For the q and k thirds, with j < d / 2,
 * m1 = M[..., j], m2 = M[..., j + d / 2], c = cosT[t, j], s = sinT[t, j]:
 *   G[..., j]         = fmaf( m2, s, m1 c)
 *   G[..., j + d / 2] = fmaf(-m1, s, m2 c)
 * (the transpose of y1 = x1 c - x2 s, y2 = x2 c + x1 s).  The v third is copied bit for bit.  G may be M itself (in place; no other
 * overlap).  No sine or cosine is evaluated: the tables are the fp32 values the forward pass used. */
int vivit_rope_jac_t_f32(const float *M, const float *cosT, const float *sinT, float *G, int64_t R, int64_t T, int64_t H, int64_t d,
                         void *stream);
/* The same rule on the packed projection of grouped-query attention (vivit_amd.backend.RotaryEmbedding with num_kv_heads; call
 * site vivit_amd/kernels.py:rope_jac_t): M, G [R, T, (H + 2 Hkv) d] = H query heads | Hkv key heads | Hkv value heads of d columns
 * each.  The H + Hkv heads of the q and k parts are rotated back by the formula above, the Hkv d columns of the v part are copied
 * bit for bit; G may be M itself.  Hkv <= 0 or H % Hkv != 0: VIVIT_E_BADARG.  vivit_rope_jac_t_f32 is this entry point with
 * Hkv = H.  VIVIT_E_UNSUPPORTED (nothing launched) for (H + 2 Hkv) d, R T or T d above 2^31 - 1. */
int vivit_rope_gqa_jac_t_f32(const float *M, const float *cosT, const float *sinT, float *G, int64_t R, int64_t T, int64_t H,
                             int64_t Hkv, int64_t d, void *stream);
/* Scaled dot-product self-attention on the packed projection (attention.hip; no counterpart in the reference's module map -- it
 * replaces the generic rule of the factor provider, a recomputed forward and torch.autograd.grad(..., is_grads_batched=True) at
 * vivit_amd/backend/extensions.py:_jac_t_mat_prod, for vivit_amd.backend.ScaledDotProductAttention).  The module input is
 * qkv [N, T, 3 H d] = q | k | v with head h in columns h d .. (h + 1) d of each third, its output out [N, T, H d].  Per factor row
 * v, sample n and head h, with dO = M[v, n, :, h]:
 *   S = scale Q K^T (causal != 0: entries j > i masked),  P = softmax_rows(S),  D_i = sum_c dO_ic out_ic,
 *   dV = P^T dO,  dP = dO V^T,  dS = P o (dP - D),  dQ = scale dS K,  dK = scale dS^T Q,   G[v, n] = dQ | dK | dV (packed as qkv).
 * No T x T data is written to memory: the workspace holds the row log-sum-exp [N, H, T] and D [V, N, H, T]; the tiles of P are
 * recomputed from it, once per workgroup for the factor rows it handles.  fp32 throughout (products on the fp32 matrix pipe), exp
 * only of arguments from which the row maximum or the row log-sum-exp has been subtracted.  No atomics and a fixed summation
 * order: the bytes of G[v, n] do not depend on V, N or the position of v and n.  Any T, H, V, N >= 1 and 1 <= d <= 128;
 * VIVIT_E_UNSUPPORTED (nothing launched) for d > 128, for more chunks of factor rows than the launch grid's second dimension takes
 * (a workgroup handles 2 rows for d > 32 and 4 otherwise, 65535 chunks: V above 131070 or 262140), and for sizes beyond the
 * kernels' index arithmetic (3 H d, N H ceil(T / 32) or V N H T / 256 above 2^31 - 1, N H T above 2^40). */
size_t vivit_attention_jac_t_f32_workspace_bytes(int64_t V, int64_t N, int64_t T, int64_t H, int64_t d);
int vivit_attention_jac_t_f32(const float *M, const float *qkv, const float *out, float *G, int64_t V, int64_t N, int64_t T,
                              int64_t H, int64_t d, float scale, int causal, void *workspace, size_t workspace_bytes,
                              void *stream);
/* Grouped-query attention: the same rule when H query heads share Hkv key / value heads (attention.hip; call site
 * vivit_amd/kernels.py:attention_jac_t with num_kv_heads, for vivit_amd.backend.ScaledDotProductAttention(num_kv_heads=...)).
 * qkv [N, T, (H + 2 Hkv) d] = q | k | v: q is the first H d columns, k the next Hkv d, v the last Hkv d; query head h attends to
 * key / value head g = h / R, R = H / Hkv consecutive query heads per group (Hkv == H: the layout above, Hkv == 1: multi-query
 * attention).  out and M [V, N, T, H d] as above, G [V, N, T, (H + 2 Hkv) d] = dQ | dK | dV packed as qkv.  Per query head h of
 * group g, S, P, D, dP, dS and dQ_h are the formulas above with K_g and V_g as operands, and
 *   dV_g = sum_{h in g} P_h^T dO_h,     dK_g = scale sum_{h in g} dS_h^T Q_h.
 * One workgroup owns a block of 32 keys of one (n, g): it walks the query heads g R .. g R + R - 1 in ascending order and inside
 * each head the query blocks in ascending order, and accumulates into one set of registers.  The summation order of every element
 * of dK and dV is therefore head, then query block, then k within the block: no atomics, no second pass, and the bytes of G[v, n]
 * depend on (T, H, Hkv, d, scale, causal) and the data of (v, n) only.  The workspace is counted in QUERY heads, lse [N, H, T] and
 * D [V, N, H, T], the same number of bytes as vivit_attention_jac_t_f32_workspace_bytes(V, N, T, H, d); the query returns 0 for
 * arguments the entry point refuses.  Hkv <= 0 or H % Hkv != 0: VIVIT_E_BADARG.  VIVIT_E_UNSUPPORTED (nothing launched, and
 * before the workspace is looked at) for d > 128, for the chunk limit above, and for sizes beyond the kernels' index arithmetic
 * ((H + 2 Hkv) d, N H ceil(T / 32), N Hkv ceil(T / 32) or V N H T / 256 above 2^31 - 1, N H T above 2^40).
 * vivit_attention_jac_t_f32 and its workspace query are these two entry points with Hkv = H. */
size_t vivit_attention_gqa_jac_t_f32_workspace_bytes(int64_t V, int64_t N, int64_t T, int64_t H, int64_t Hkv, int64_t d);
int vivit_attention_gqa_jac_t_f32(const float *M, const float *qkv, const float *out, float *G, int64_t V, int64_t N, int64_t T,
                                  int64_t H, int64_t Hkv, int64_t d, float scale, int causal, void *workspace,
                                  size_t workspace_bytes, void *stream);
/* The same rule with per-sample sequence lengths and a sliding window; the two entry points above are this one with lengths = NULL
 * and window = 0, byte for byte.  lengths [N] int32 on the device (NULL: every sample has T positions): sample n has
 * Tn = min(max(lengths[n], 0), T) live positions 0 .. Tn - 1 (right padding; the kernels clamp, so no value can carry an access out
 * of bounds).  window W >= 1 (0: none; W >= T is the same function as none, values above 2^31 - 1 included; W < 0: VIVIT_E_BADARG).
 * Query i sees key j iff i < Tn and j < Tn, j <= i when causal, and i - j < W and j - i < W when W > 0: with causal the W keys
 * i - W + 1 .. i, the query's own position included.  Positions t >= Tn are dead: as keys invisible, as queries without output, rows
 * t >= Tn of G[v, n] are written as +0, and the data of M, qkv and out there is never loaded (NaN there reaches nothing).  Only the
 * 32 x 32 tiles with a visible pair are visited, in the order above, so G[v, n, :Tn] has the bytes of the call on sample n cut to Tn
 * positions with T = Tn, whatever the other samples' lengths.  The workspace is that of the grouped-query entry point. */
size_t vivit_attention_masked_jac_t_f32_workspace_bytes(int64_t V, int64_t N, int64_t T, int64_t H, int64_t Hkv, int64_t d);
int vivit_attention_masked_jac_t_f32(const float *M, const float *qkv, const float *out, float *G, int64_t V, int64_t N, int64_t T,
                                     int64_t H, int64_t Hkv, int64_t d, float scale, int causal, const int32_t *lengths,
                                     int64_t window, void *workspace, size_t workspace_bytes, void *stream);
/* The same rule for a modified score function (attention.hip; call site vivit_amd/kernels.py:attention_jac_t with softcap or bias, for
 * vivit_amd.backend.ScaledDotProductAttention(softcap=, bias=)): a logit cap and an additive bias per head and distance.  With
 * z_ij = scale q_i k_j:  u = c tanh(z / c) for softcap c > 0 (softcap == 0: u = z; Gemma-2, Grok-1),  s_ij = u + bias[h, j - i + T - 1]
 * for bias [H, 2 T - 1] fp32 on the device (NULL: s = u; ALiBi, relative-position tables), then the mask of the masked entry point
 * exactly as it is, P = softmax_rows(s): the cap comes before the bias and the mask.  The rule:  dS = P o (dP - D),
 * dZ = dS o (1 - t^2) with t = u / c (no cap: dZ = dS),  dQ_h = scale dZ K_g,  dK_g = scale sum_{h in g} dZ_h^T Q_h,  dV as above.  The
 * table is a constant and receives no factor.  Only entries of visible pairs are read, both positions < Tn <= T, so no index leaves
 * [0, 2 T - 2]; the table needs no alignment beyond its four bytes.  Tiles, block ranges, summation orders, dead positions and +0
 * rows are those of the masked entry point, no atomics, no T x T data in memory; the bytes of G[v, n] depend on the shape parameters,
 * the cap, the table and the data of (v, n) only.  With softcap == 0 and bias == NULL the call IS
 * vivit_attention_masked_jac_t_f32 (it is forwarded: the same kernels, the same bytes).  softcap negative, NaN or inf:
 * VIVIT_E_BADARG; every other refusal (BADARG, UNSUPPORTED, WORKSPACE) is that of the masked entry point, and all come before any
 * launch.  The workspace is that of the masked entry point.  There is no such entry for cross-attention. */
size_t vivit_attention_scoremod_jac_t_f32_workspace_bytes(int64_t V, int64_t N, int64_t T, int64_t H, int64_t Hkv, int64_t d);
int vivit_attention_scoremod_jac_t_f32(const float *M, const float *qkv, const float *out, float *G, int64_t V, int64_t N, int64_t T,
                                       int64_t H, int64_t Hkv, int64_t d, float scale, int causal, const int32_t *lengths,
                                       int64_t window, float softcap, const float *bias, void *workspace, size_t workspace_bytes,
                                       void *stream);
/* The factor of a LEARNED bias table (attention.hip; call site vivit_amd/kernels.py:attention_bias_factor, for
 * vivit_amd.backend.ScaledDotProductAttention(bias=, learn_bias=True)): the transposed Jacobian of the function of the score-modifier
 * entry point with respect to its table, applied to M.  Per factor row v, sample n and query head h,
 *   Gb[v, n, h, b] = sum over the distances r = j - i with index[r + T - 1] == b of  sum_{(i, j) visible, j - i = r} dS[v, n, h, i, j],
 * dS = P o (dP - D) of that entry point: the table is added behind the cap, so it is dS and not dZ that is summed.  bias [H, 2 T - 1]
 * fp32 on the device is the EFFECTIVE table of the T positions (not NULL); index [2 T - 1] int32 on the device (not NULL) sends the
 * distance r to column index[r + T - 1] of Gb [V, N, H, R] (fp32, dense, uninitialised memory: every element has exactly one writer).
 * A plain table built for L >= T positions: index[k] = k + (L - T), R = 2 L - 1; a table indexed through buckets (T5): the middle
 * slice of the bucket map, R the number of buckets.  The index is never read on the host and its values cannot be checked: a value
 * outside [0, R) is SKIPPED by the fold (it equals no column), so that no value can carry a store out of bounds -- the distance then
 * contributes to no column.  lengths, window, softcap, scale and causal are those of the score-modifier entry point.
 * Launches: the row log-sum-exp and the row dots as that entry point has them, then the DIAGONAL OWNER -- one workgroup per block
 * diagonal delta = jb - ib of one (n, h) and chunk of factor rows walks the query blocks ib in ascending order over exactly the tiles
 * (ib, ib + delta) that the block ranges above call non-empty, recomputes dS per tile, and adds its 63 diagonals rho = -31 .. 31
 * (i ascending inside a tile) into registers that live across the walk; it writes partial[v, n, h, delta, rho] -- and a fold: a
 * distance r lies on the block diagonals floor(r / 32) (at rho = r mod 32) and, for rho >= 1, the next one (at rho - 32);
 * Gb[v, n, h, b] is ONE chain of sums over r ascending, each r the sum of its two block diagonals (delta ascending).  No atomics; the bytes of Gb[v, n] depend
 * on the shape parameters, the cap, the table, the index and the data of (v, n) only; a padded sample has the bytes of the sample
 * cut to Tn and run alone with the index shifted by T - Tn; no operand row of a dead position is loaded; a column that no visible
 * distance maps to, and every column of a dead sample, is written as +0.  No T x T data in memory.
 * Workspace: that of the score-modifier entry point followed by the partial sums [V, N, H, 2 ceil(T / 32) - 1, 64] fp32, i.e.
 * 4 * 64 * (2 ceil(T / 32) - 1) bytes more per (v, n, h); the query returns 0 for arguments the entry point refuses.
 * VIVIT_E_BADARG: bias == NULL, index == NULL, R < 1, and what the score-modifier entry point refuses so; VIVIT_E_UNSUPPORTED: as
 * there, and N H (2 ceil(T / 32) - 1) above 2^31 - 1 (the diagonal owner's grid); VIVIT_E_WORKSPACE: a missing or short workspace.
 * Every refusal comes before any launch. */
size_t vivit_attention_bias_factor_f32_workspace_bytes(int64_t V, int64_t N, int64_t T, int64_t H, int64_t Hkv, int64_t d);
int vivit_attention_bias_factor_f32(const float *M, const float *qkv, const float *out, float *Gb, int64_t V, int64_t N, int64_t T,
                                    int64_t H, int64_t Hkv, int64_t d, float scale, int causal, const int32_t *lengths,
                                    int64_t window, float softcap, const float *bias, const int32_t *index, int64_t R,
                                    void *workspace, size_t workspace_bytes, void *stream);
/* Cross-attention: the same rule when the queries and the keys come from two sequences (attention.hip; call site
 * vivit_amd/kernels.py:cross_attention_jac_t, for vivit_amd.backend.ScaledDotProductCrossAttention).  All tensors dense:
 * q [N, Tq, H d], kv [N, Tk, 2 Hkv d] = k | v (Hkv key heads of d columns, then Hkv value heads: the packed layout above without
 * its query part), out and M [V, N, Tq, H d]; Gq [V, N, Tq, H d] = dQ and Gkv [V, N, Tk, 2 Hkv d] = dK | dV.  Query head h uses key /
 * value head h / (H / Hkv).  There is NO causal flag and NO window: with Tq != Tk there is no agreed alignment of the diagonal.
 * q_lengths, k_lengths [N] int32 on the device, either may be NULL (every sample has Tq / Tk positions): right padding, clamped in
 * the kernels to Lq in [0, Tq] and Lk in [0, Tk].  Key j of sample n is live iff j < Lk[n]; query i is live iff i < Lq[n] AND
 * Lk[n] > 0 (a query with no key to look at is dead, it is not a NaN); a live query sees every live key.  The rows of the dead
 * positions of Gq and Gkv are written as +0, no operand row of a dead position is ever loaded (NaN there reaches nothing), and only
 * the 32 x 32 tiles with a live pair are visited.  Gq or Gkv may be NULL, not both (VIVIT_E_BADARG): the owner of a NULL result is
 * not launched -- Gkv == NULL (a frozen memory) skips the key-block owner, Gq == NULL the query-block owner; the lse and row-dot
 * launches serve either.  The summation orders are those above (dK, dV: query heads of the group ascending, query blocks
 * ascending, k within the block ascending; dQ: key blocks ascending), no atomics, no second pass, no Tq x Tk data in memory: the
 * bytes of G[v, n] depend on (Tq, Tk, H, Hkv, d, scale), the two lengths of n and the data of (v, n) only; with Tq = Tk, equal
 * lengths and q | kv one packed projection they are those of vivit_attention_masked_jac_t_f32 with causal = 0 and window = 0, and
 * sample n has the bytes of the call on that sample cut to (Lq, Lk) without lengths.  The workspace, lse [N, H, Tq] and
 * D [V, N, H, Tq], is vivit_attention_gqa_jac_t_f32_workspace_bytes(V, N, Tq, H, Hkv, d) bytes, whatever Tk; the query returns 0 for
 * arguments the entry point refuses.  VIVIT_E_BADARG: non-positive sizes, H % Hkv != 0, a null operand, both results null.
 * VIVIT_E_UNSUPPORTED (nothing launched, and before the workspace is looked at): d > 128, the chunk limit above, and sizes beyond
 * the kernels' index arithmetic (the pitches H d and 2 Hkv d -- (H + 2 Hkv) d is what is checked --, the block counts
 * N H ceil(Tq / 32) and N Hkv ceil(Tk / 32), or V N H Tq / 256 above 2^31 - 1; N H Tq or N Hkv Tk above 2^40).  VIVIT_E_WORKSPACE: a
 * missing or short workspace. */
size_t vivit_attention_cross_jac_t_f32_workspace_bytes(int64_t V, int64_t N, int64_t Tq, int64_t Tk, int64_t H, int64_t Hkv,
                                                       int64_t d);
int vivit_attention_cross_jac_t_f32(const float *M, const float *q, const float *kv, const float *out, float *Gq, float *Gkv,
                                    int64_t V, int64_t N, int64_t Tq, int64_t Tk, int64_t H, int64_t Hkv, int64_t d, float scale,
                                    const int32_t *q_lengths, const int32_t *k_lengths, void *workspace, size_t workspace_bytes,
                                    void *stream);
/* nn.Embedding (embedding.hip; the reference has no rule for it): the weight factor Vt[v, n, w, :] = sum_{t: idx[n, t] = w} M[v, n, t, :]
 * of the factor M [V, N, T, D] at the module output has at most T non-zero rows per (v, n) out of W = num_embeddings and is kept
 * compact: ids [N, T] int32 holds sample n's distinct tokens in strictly increasing order in its first U_n slots and -1 in the rest,
 * B [V, N, T, D] the sum of the rows of M[v, n] per slot (rows of -1 slots are zero).  fp32, no atomics, fixed summation orders.
 * Every entry point: VIVIT_E_BADARG for a null pointer or a non-positive size, VIVIT_E_UNSUPPORTED (nothing launched) for sizes
 * beyond the kernels' 32-bit index arithmetic (any size, D + 128 or N (T + 1) + 256 above 2^31 - 1, V N T D above 2^39 - 256).
 *
 * vivit_embedding_compact_f32 (vivit_amd/kernels.py:embedding_compact, which sorts each sample's tokens with torch): perm [N, T] are
 * the positions t of sample n ordered by token, stably; slot u owns the seg_count[n, u] sorted positions from seg_start[n, u] on:
 *   B[v, n, u, :] = sum_{j < seg_count[n, u]} M[v, n, perm[n, seg_start[n, u] + j], :]      (ascending j, i.e. ascending t) */
int vivit_embedding_compact_f32(const float *M, const int32_t *perm, const int32_t *seg_start, const int32_t *seg_count, float *B,
                                int64_t V, int64_t N, int64_t T, int64_t D, void *stream);
/* The Gram matrix of the weight factor from its compact form (vivit_amd/backend/extensions.py:_embedding_closures, gram_mat):
 *   G[v N + n, v' N + n'] = alpha sum_{u, u'} [ids[n, u] = ids[n', u'] >= 0] <B[v, n, u, :], B[v', n', u', :]> + beta G[..]
 * G [V N, V N] contiguous; beta == 0: G is not read.  Output-stationary on v_mfma_f32_16x16x4_f32: a workgroup owns a pair of
 * 16-sample blocks and 4 x 4 classes and walks the tokens the two blocks share in ascending order.  The bytes of a sample pair's
 * V x V block depend on the two samples only; samples without a common token give exact zeros (for finite B: a sample that lacks a token of
 * its block enters with a zero row, and 0 x inf is NaN); entries on and below the diagonal
 * are computed and written to both positions, so alpha-term and result are exactly symmetric (for a symmetric G when beta != 0).
 * Workspace: the token tables of the sample blocks, 4 (2 N T + N + 17 * 16 ceil(N / 16) T) bytes and alignment -- nothing of size
 * W, (N T)^2 or per token.  VIVIT_E_UNSUPPORTED also for N above 16 * 65535 (the pairs of sample blocks are the grid's first dimension), V above 1020 or V N
 * above 2^31 - 1. */
size_t vivit_embedding_gram_f32_workspace_bytes(int64_t V, int64_t N, int64_t T, int64_t D);
int vivit_embedding_gram_f32(const float *B, const int32_t *ids, float *G, int64_t V, int64_t N, int64_t T, int64_t D, float alpha,
                             float beta, void *workspace, size_t workspace_bytes, void *stream);
/* V_mat_prod of the closures: out[f, w, :] = sum_{v, n, u: ids[n, u] = w} mat[f, v, n] B[v, n, u, :], out [F, W, D], mat [F, V, N].
 * order [N T] int32: the entries n T + u stably sorted by token (vivit_amd/kernels.py:embedding_vmp sorts with torch); token w owns
 * the positions tok_start[w] .. tok_start[w + 1] (tok_start [W + 1]).  One wave per (w, f) sums its members in that order; rows of
 * absent tokens are zero.  VIVIT_E_UNSUPPORTED also for F above 65535. */
int vivit_embedding_vmp_f32(const float *B, const int32_t *order, const int32_t *tok_start, const float *mat, float *out, int64_t F,
                            int64_t V, int64_t N, int64_t T, int64_t D, int64_t W, void *stream);
/* V_t_mat_prod of the closures: out[f, v, n] = sum_u <mat[f, ids[n, u], :], B[v, n, u, :]>, mat [F, W, D], out [F, V, N]; ids outside
 * [0, W) are skipped.  VIVIT_E_UNSUPPORTED also for F V N above 2^31 - 1. */
int vivit_embedding_vtmp_f32(const float *B, const int32_t *ids, const float *mat, float *out, int64_t F, int64_t V, int64_t N,
                             int64_t T, int64_t D, int64_t W, void *stream);
/* The explicit factor (vivit_amd/backend/extensions.py:_param_factor, and factor() of the closures): out [V, N, W, D] = zeros, then
 * out[v, n, ids[n, u], :] = B[v, n, u, :] for ids[n, u] in [0, W).  VIVIT_E_UNSUPPORTED also for V N W D above 2^60. */
int vivit_embedding_weight_mjp_f32(const float *B, const int32_t *ids, float *out, int64_t V, int64_t N, int64_t T, int64_t D,
                                   int64_t W, void *stream);
/* Cross-entropy loss-Hessian square root from the logits [N, C]: p = softmax.  onehot == NULL (exact, V must equal C):
 * S[v, n, c] = sqrt(p_nv) (delta_vc - p_nc) scale;  onehot [V, N, C] (sampled): S[v, n, c] = (p_nc - onehot[v, n, c]) scale. */
int vivit_ce_sqrt_hessian_f32(const float *logits, const float *onehot, float *S, int64_t N, int64_t C, int64_t V, float scale,
                              void *stream);
/* The same for outputs with positions (csrc/loss_positions.hip): N samples of C classes at L positions, sample stride C L, a softmax
 * over the classes at every position, p[n, :, l] = softmax_c(logits[n, :, l]).  layout 0 ("NCL"): class stride L, position stride 1
 * (a contiguous [N, C, *D]); layout 1 ("NLC"): class stride 1, position stride C (a contiguous [N, *D, C] seen as [N, C, *D]).
 * idx == NULL (exact, V must equal C L, row v = c' L + l'):  S[v, n, c, l] = [l = l'] sqrt(p[n, c', l]) ([c = c'] - p[n, c, l]) scale;
 * idx [V, N, L] int32 class indices (sampled):               S[m, n, c, l] = (p[n, c, l] - [c = idx[m, n, l]]) scale.
 * Every (v, n) slice of S has the layout of a sample of the logits; every element is written, the zeros of the exact factor included.
 * An index outside [0, C) matches no class: that position of the slice is p scale, and no address is formed from an index.
 * Non-finite logits follow torch.softmax: -inf beside finite classes is p = 0; a NaN or +inf at any class of a position, or -inf at
 * all of them, makes every class of that position NaN in every slice that writes it, and changes no other position.  C has no
 * upper limit other than the index arithmetic.  Any zero size: VIVIT_OK, no pointer is read.  VIVIT_E_BADARG: a negative size, layout
 * other than 0 or 1, logits or S null, exact with V != C L.  VIVIT_E_UNSUPPORTED: a size or N L above 2^31 - 1, V N C L above 2^60. */
int vivit_ce_pos_sqrt_hessian_f32(const float *logits, const int32_t *idx, float *S, int64_t N, int64_t C, int64_t L, int64_t V, int layout,
                                  float scale, void *stream);
/* The two factors above with one scale per position instead of one float, for cross entropy with ignore_index, class weights and
 * label smoothing: the loss Hessian at position i = (n, l) is omega_i (diag p_i - p_i p_i^T), and the factors are those above times
 * s_i = sqrt(omega_i) (exact) or sqrt(omega_i / M) (sampled) at position i.  pos_scale [N L] (row n L + l; row_scale [N] for the
 * [N, C] kernel) holds s_i; it enters where `scale` enters above, (p - e) * s and sqrtf(p) * s with the same operations in the same
 * order, so an array whose elements all hold one float s gives the bytes of the entry point above called with scale = s.
 * A position with s == 0 is written as exact zeros in every slice that covers it, whatever its logits hold (NaN and +-inf included:
 * padded positions carry garbage); in layout 1 and in the [N, C] kernel its logits are not read.  A position with s != 0 follows the
 * non-finite rules above.  Status codes, zero sizes and limits as above; pos_scale / row_scale null is VIVIT_E_BADARG. */
int vivit_ce_pos_sqrt_hessian_w_f32(const float *logits, const int32_t *idx, const float *pos_scale, float *S, int64_t N, int64_t C,
                                    int64_t L, int64_t V, int layout, void *stream);
int vivit_ce_sqrt_hessian_w_f32(const float *logits, const float *onehot, const float *row_scale, float *S, int64_t N, int64_t C,
                                int64_t V, void *stream);
/* pos_scale [R] of the two entry points above from class-index targets, on the device (nothing returns to the host; no atomics, two
 * calls give the same bytes).  target [R] int64 (R = N L, row r = n L + l); class_weight [C] or NULL (all ones); wbar = mean_c w_c;
 * eps = label_smoothing; mean = 1 for reduction 'mean', 0 for 'sum'; mult = M for the sampled factor, 1 for the exact one.
 *   counted_r = target[r] != ignore_index and 0 <= target[r] < C
 *   a_r       = counted_r ? (1 - eps) w[target[r]] + eps wbar : 0          (exactly 1 without weights)
 *   norm      = mean ? sum over the counted rows of w[target[r]] : 1       (over all R rows: before any sub-sampling)
 *   pos_scale[r] = (float)(sqrt(a_r) / sqrt(mult norm)),  evaluated in fp64 in exactly this form: with no weights and nothing
 *   ignored it is the float 1 / sqrt(mult R) that the unweighted entry points are handed as `scale`.
 * norm and wbar are fp64 sums in a fixed order (per-workgroup partials in the workspace, added in index order).
 * Decisions: a_r == 0 gives 0, also when norm == 0 (every target ignored: the factor is zero where torch's loss is NaN); a_r < 0
 * (negative class weights) gives NaN at that row; a target outside [0, C) other than ignore_index has weight 0, and no address is
 * formed from it.  R == 0: VIVIT_OK, no pointer is read.  VIVIT_E_BADARG: R or C negative, mult < 1, mean outside {0, 1}, target or
 * pos_scale null.  VIVIT_E_UNSUPPORTED: R, C or mult above 2^31 - 1.  VIVIT_E_WORKSPACE: workspace null, not 8-byte aligned or
 * smaller than vivit_ce_target_scales_f32_workspace_bytes(R, C). */
size_t vivit_ce_target_scales_f32_workspace_bytes(int64_t R, int64_t C);
int vivit_ce_target_scales_f32(const int64_t *target, const float *class_weight, float *pos_scale, int64_t R, int64_t C, int64_t ignore_index,
                               double label_smoothing, int mean, int64_t mult, void *workspace, size_t workspace_bytes, void *stream);

/* ---------------------------------------------------------------------------------------------
 * K3/K4  Symmetric eigendecomposition (Householder tridiagonalisation + implicit-shift QL,
 * divide-and-conquer merges above the single-workgroup size).
 *   A: [n, n] symmetric, lda >= n.  DESTROYED (holds the Householder reflectors on return).
 *      Only the lower triangle (A[i][j], i >= j) is read.
 *   w: [n] eigenvalues, ascending.
 *   Z: [n, n] ldz >= n or NULL.  Z[:, i] is the unit eigenvector of w[i] (column-wise, as
 *      Tensor.symeig returned them: vivit/utils/eig.py:24-26).  NULL = values only.
 *   info: device int32; 0 on success, >0 = number of unconverged eigenvalues.
 * INPUT RANGE (tests/test_symeig_scale_gpu.py, tests/test_symeig_degenerate_gpu.py; every entry point of this section, the
 *   batched, row-range, banded and reduce / select ones included).  With amax = max |a_ij| inside 2^-20 .. 2^51 the matrix is
 *   used as it is; outside, it is multiplied by a power of two (exact) -- the one that brings amax into [1, 2), limited to
 *   2^-126 .. 2^127, so that a denormal amax ends below 1 and an amax of 2^127 or more in [2, 4) -- and the eigenvalues
 *   are divided by it at the end (exact unless they leave the normal range).  The stated accuracy -- eigenvalues to 1e-5
 *   ||A||_2, Z^T Z - I to 5e-5, A Z - Z diag(w) to 3e-5 ||A||_2 (2e-5, 2e-5, 5e-5 at n <= 192) -- is tested with amax at
 *   2^-120, on both sides of 2^-51, of 2^-20 (the edge) and of 2^51, at 2^-10 and order n (unscaled) and at 2^100, for
 *   ||A||_2 up to 2^126, each problem of a batch on its own scale, and on the zero matrix, c I (exact), diagonal,
 *   tridiagonal, block-diagonal and rank-one input, with info = 0.  A matrix whose entries are all denormal
 *   (amax = 2^-130) meets the same bounds plus n 2^-149, the spacing of its own entries.  An eigenvalue beyond FLT_MAX
 *   comes back as +-inf with info = 0, the other eigenvalues and Z finite.  An entry above 3.0e38 or a non-finite one
 *   gives info = n.  vivit_stedc_f32 on its own is tested for max(|d|, |e|) from 2^-50 to 2^50.
 * Replaces Tensor.symeig(eigenvectors=False)  vivit/linalg/eigvalsh.py:221 and
 *   Tensor.symeig(eigenvectors=True)  vivit/linalg/eigh.py:248-250,
 *   vivit/optim/directional_damped_newton.py:315, vivit/optim/directional_derivatives.py:291,
 *   vivit/utils/eig.py:38,104.
 * ------------------------------------------------------------------------------------------- */
size_t vivit_symeig_f32_workspace_bytes(int64_t n, int want_vectors);
int vivit_symeig_f32(float *A, int64_t n, int64_t lda, float *w, float *Z, int64_t ldz,
                     void *workspace, size_t workspace_bytes, int32_t *info, void *stream);

/* Eigenvalues of `batch` symmetric matrices of ONE size in one call (block-diagonal curvature: one spectrum per layer).
 *   A: HOST array of `batch` device pointers, each [n, n] with the common lda >= n; every matrix is DESTROYED, only its
 *      lower triangle is read.  The array itself is read before the call returns.
 *   W: [batch][n] device, row b = eigenvalues of A[b], ascending.   info: device int32 [batch], per problem as above.
 * Any batch >= 1: processed in waves of eight on the stream; the workspace is that of min(batch, 8) problems.
 *   n <= 192: the single-workgroup solver, one workgroup per problem, one launch per wave (no workspace).
 *   193 <= n <= 1280: the persistent tridiagonalisation with one problem per XCD in ONE launch -- a single solve of
 *     this size keeps its matrix in the registers of one XCD's 32 CUs and leaves the other seven XCDs idle.  Every
 *     problem has its own arrival gate, counters and exchange buffers; the failure word is the stream's, so if any
 *     problem's persistent kernel gives up, EVERY info word of that wave is VIVIT_INFO_PERSIST_TIMEOUT.  With the
 *     persistent kernels switched off (vivit_persistent_kernels(0), VIVIT_SYTRD_PERSIST=0): the single solve, problem
 *     after problem.
 *   n > 1280: VIVIT_E_UNSUPPORTED (those sizes use the whole chip per problem: call vivit_symeig_f32 in a loop).
 * On every route row b of W holds exactly the bytes vivit_symeig_f32(A[b], Z = NULL) writes.
 * Not in the reference, which solves one group at a time (vivit/linalg/eigvalsh.py:221). */
size_t vivit_symeigvals_batched_f32_workspace_bytes(int64_t n, int64_t batch);
int vivit_symeigvals_batched_f32(float *const *A, int64_t batch, int64_t n, int64_t lda, float *W, void *workspace,
                                 size_t workspace_bytes, int32_t *info, void *stream);

/* Row-range variant for the multi-GPU path: all n eigenvalues (ascending) plus the eigenvectors
 * row_begin .. row_end-1 (in that order) as ROWS of Zt: [row_end - row_begin, n], ldz >= n.  Reduction and
 * tridiagonal solve run in full on every caller; only the back-transformations, which act on each eigenvector
 * independently, are restricted to the requested range - R ranks that hold the same A (after the all-reduce
 * of the partial Gram matrices) each pay 1/R of that stage and exchange their slices.
 * Same workspace as vivit_symeig_f32(want_vectors = 1).  n <= 192: VIVIT_E_UNSUPPORTED (use vivit_symeig_f32).
 * Replaces the same Tensor.symeig(eigenvectors=True) call sites as vivit_symeig_f32. */
int vivit_symeig_rows_f32(float *A, int64_t n, int64_t lda, float *w, float *Zt, int64_t ldz, int64_t row_begin,
                          int64_t row_end, void *workspace, size_t workspace_bytes, int32_t *info, void *stream);

/* Two-phase variant for callers that keep only a few eigenvectors (SURVEY.md 8b `symeig_select_f32`).  The reference
 * computes all n eigenvectors and slices them with the index list its `criterion` callback returns from the
 * eigenvalues: evals, evecs = symeig(...); keep = criterion(evals); evecs[:, keep]
 *   vivit/linalg/eigh.py:248-253, vivit/optim/directional_damped_newton.py:315-321,
 *   vivit/optim/directional_derivatives.py:291-297.
 * Here the callback runs between two calls:
 *   vivit_symeig_reduce_f32: A (destroyed, as in vivit_symeig_f32) -> tridiagonal form; w: all n eigenvalues,
 *     ascending (Sturm multisection).  `state` (vivit_symeig_reduce_f32_workspace_bytes(n) bytes) receives the
 *     tridiagonal, the fp64 eigenvalues, the reflector scalars and the second-stage reflectors; A keeps the
 *     first-stage reflectors.  Neither may be touched before phase 2.
 *   vivit_symeig_select_f32: idx: DEVICE int32 [K], strictly ascending positions into w; Zt: [K, n] (ldz >= n),
 *     row k = unit eigenvector of w[idx[k]].  K <= 256: inverse iteration on the tridiagonal (fp64), else divide &
 *     conquer; then only those K rows are back-transformed (4 K n^2 flop instead of 4 n^3).  May be called more than
 *     once per reduction.  Same (A, n, lda, state) as phase 1; `workspace` is scratch of
 *     vivit_symeig_select_f32_workspace_bytes(n, K) bytes.
 * n <= 192: VIVIT_E_UNSUPPORTED (use vivit_symeig_f32 and slice). */
size_t vivit_symeig_reduce_f32_workspace_bytes(int64_t n);
size_t vivit_symeig_select_f32_workspace_bytes(int64_t n, int64_t K);
int vivit_symeig_reduce_f32(float *A, int64_t n, int64_t lda, float *w, void *state, size_t state_bytes,
                            int32_t *info, void *stream);
int vivit_symeig_select_f32(const float *A, int64_t n, int64_t lda, const int32_t *idx, int64_t K, float *Zt, int64_t ldz,
                            void *state, size_t state_bytes, void *workspace, size_t workspace_bytes, int32_t *info,
                            void *stream);

/* The two phases for `batch` symmetric matrices of ONE size 193 <= n <= 1280 (block-diagonal curvature: one group per
 * layer, each with its own criterion callback between the calls -- the per-group loop around vivit/linalg/eigh.py:248-253).
 * Any batch >= 1, in waves of eight on the stream; the number of launches of a wave does not depend on how many problems
 * it holds.  A, Zt, state, K: HOST arrays of `batch` entries, read before the call returns.
 *   vivit_symeig_reduce_batched_f32: A[b] as in vivit_symeig_reduce_f32 (destroyed; keeps the reflectors).  W: [batch][n]
 *     device, row b ascending.  state[b]: DEVICE block of state_bytes_each >= vivit_symeig_reduce_f32_workspace_bytes(n)
 *     bytes.  One persistent tridiagonalisation launch (problem q on XCD q) and one Sturm multisection launch per wave.
 *     Afterwards (A[b], state[b]) is exactly what vivit_symeig_reduce_f32 leaves and row b of W has its bytes: problem b may
 *     be continued with vivit_symeig_select_f32.  info: device int32 [batch]; non-finite input fails only its own problem
 *     (info[b] = n); a persistent kernel that gives up voids the wave (every word VIVIT_INFO_PERSIST_TIMEOUT).  With the
 *     persistent kernels off or the two-stage reduction forced: vivit_symeig_reduce_f32 problem after problem.
 *   vivit_symeig_select_batched_f32: idx: DEVICE int32, the selections of all problems one after the other (K[0], then K[1],
 *     ... entries; strictly ascending within a problem); K[b] (HOST, 0 <= K[b] <= n) may differ, 0 is legal.  Zt[b]: DEVICE
 *     [K[b]][ldz >= n], row k = unit eigenvector of problem b for W[b][idx_b[k]] (may be NULL when K[b] = 0).  Per wave:
 *     three launches of inverse iteration over all (problem, eigenvalue) pairs and ONE launch that applies every problem's
 *     Householder reflectors to its rows (one wavefront per row, reflector by reflector -- not the compact-WY products of
 *     the single select, so the vectors agree with vivit_symeig_select_f32 to rounding, not bit for bit; a problem's rows do
 *     not depend on what else is in the batch).  A problem with K[b] > 256 leaves the wave and goes through
 *     vivit_symeig_select_f32.  workspace: vivit_symeig_select_batched_f32_workspace_bytes(n, batch, max K[b]) bytes, constant
 *     beyond eight problems.
 * n <= 192 and n > 1280: VIVIT_E_UNSUPPORTED (loop over the single entry points).  Not in the reference. */
size_t vivit_symeig_select_batched_f32_workspace_bytes(int64_t n, int64_t batch, int64_t K_max);
int vivit_symeig_reduce_batched_f32(float *const *A, int64_t batch, int64_t n, int64_t lda, float *W, void *const *state,
                                    size_t state_bytes_each, int32_t *info, void *stream);
int vivit_symeig_select_batched_f32(const float *const *A, int64_t batch, int64_t n, int64_t lda, const int32_t *idx,
                                    const int64_t *K, float *const *Zt, int64_t ldz, void *const *state,
                                    size_t state_bytes_each, void *workspace, size_t workspace_bytes, int32_t *info,
                                    void *stream);

/* Stage 1 of vivit_symeig_f32, exported for testing: Householder tridiagonalisation
 * A = Q T Q^T (lower triangle read).  d: [n], e: [n-1], tau: [n]; on return row j of A's upper
 * triangle, A[j][j+1:], holds reflector v_j (v_j[j+1] = 1), Q = H_0 ... H_{n-3},
 * H_j = I - tau[j] v_j v_j^T.  n >= 3. */
size_t vivit_sytrd_f32_workspace_bytes(int64_t n);
int vivit_sytrd_f32(float *A, int64_t n, int64_t lda, float *d, float *e, float *tau,
                    void *workspace, size_t workspace_bytes, void *stream);

/* Stage 1a of the two-stage path, exported for testing: full symmetric A (BOTH triangles valid,
 * lda >= n) -> symmetric band with half bandwidth vivit_sb2st_half_bandwidth() by blocked
 * Householder QR of the sub-band panels and two-sided MFMA updates.  On return the band is in A
 * (A[i][j], 0 <= i-j <= NB) and, copied, in AB ([n][2*NB+1] row-band layout); reflector c of
 * panel p sits in A[p*NB + c][(p+1)*NB + c ..]; tau1: [n]. */
size_t vivit_sy2sb_f32_workspace_bytes(int64_t n);
int vivit_sy2sb_f32(float *A, int64_t n, int64_t lda, float *AB, float *tau1, void *workspace,
                    size_t workspace_bytes, void *stream);

/* The pieces of the two-stage solver around a band reduction that is done by the CALLER -- the multi-GPU path
 * (vivit_amd/distributed.py:sy2sb_sharded): the trailing matrix is sharded by block columns over the
 * ranks, the sub-band panel is broadcast and factored by every rank, the rest of the solve runs as in
 * vivit_symeig_rows_f32.
 *   vivit_symeig_prepare_f32: LAPACK-style scaling of A + mirror of the lower triangle (A then has BOTH triangles);
 *     scal: DEVICE float[16] (scal[1] = the factor applied, scal[2] = non-finite-input flag), to be handed to
 *     vivit_symeig_banded_rows_f32.  workspace: 8 n + 256 bytes.
 *   vivit_sy2sb_panel_qr_f32: Householder QR of one panel, pan: [mp][NB] row-major (NB = vivit_sb2st_half_bandwidth()),
 *     factored in place: R's strict upper triangle in rows 0..NB-1, its diagonal in betas[NB].  Vt: [NB][ldv] receives
 *     the reflectors as ROWS (Vt[c][r] = v_c[r], v_c[c] = 1, zeros in front), tau: [NB], T: [NB][NB] upper triangular
 *     with Q = I - V T V^T (LAPACK larft, forward / columnwise).
 *   vivit_symeig_banded_rows_f32: A as vivit_sy2sb_f32 leaves it (band in A[i][j], 0 <= i-j <= NB; reflector c of
 *     panel p in A[p*NB + c][(p+1)*NB + c ..]), tau1: DEVICE [n]; continues with bulge chasing, divide & conquer and the
 *     two back-transformations restricted to the eigenvectors row_begin .. row_end-1 (ROWS of Zt, as
 *     vivit_symeig_rows_f32).  Workspace of vivit_symeig_f32(want_vectors = 1).  n > 2 NB.
 * Replace the same Tensor.symeig(eigenvectors=True) call sites as vivit_symeig_f32. */
int vivit_symeig_prepare_f32(float *A, int64_t n, int64_t lda, float *scal, void *workspace, size_t workspace_bytes,
                             void *stream);
size_t vivit_sy2sb_panel_qr_f32_workspace_bytes(int64_t mp);
int vivit_sy2sb_panel_qr_f32(float *pan, int64_t mp, float *Vt, int64_t ldv, float *tau, float *betas, float *T,
                             void *workspace, size_t workspace_bytes, void *stream);
int vivit_symeig_banded_rows_f32(float *A, int64_t n, int64_t lda, const float *tau1, const float *scal, float *w,
                                 float *Zt, int64_t ldz, int64_t row_begin, int64_t row_end, void *workspace,
                                 size_t workspace_bytes, int32_t *info, void *stream);

/* Stage 1b of the two-stage path, exported for testing: symmetric BAND -> tridiagonal by bulge
 * chasing.  Half bandwidth NB = vivit_sb2st_half_bandwidth() (64).  AB: [n][2*NB+1] row-band
 * layout, AB[i][j - i + 2*NB] = A[i][j] for i - 2*NB <= j <= i (entries with i - j > NB must be
 * zero on entry: bulge room); contents unspecified afterwards (the chase runs on a copy with padded
 * rows inside the workspace).  d: [n], e: [n].  R2: [n][n], row s receives the
 * Householder vectors of sweep s (for the back-transformation). */
int vivit_sb2st_half_bandwidth(void);
size_t vivit_sb2st_f32_workspace_bytes(int64_t n);
int vivit_sb2st_f32(float *AB, int64_t n, float *d, float *e, float *R2, void *workspace,
                    size_t workspace_bytes, void *stream);

/* Stage 3a of the two-stage path, exported for testing: the back-transformation through the bulge-chasing reflectors,
 *   Zt <- Zt * Q2^T,   Q2 = product of all H(s, k) = I - tau2[s][k] v(s,k) v(s,k)^T in generation order,
 * Zt: [nrows][ldz] (rows = eigenvectors of the tridiagonal matrix on entry, of the band matrix on return; any subset of
 * rows: rows are independent), R2 / tau2 as vivit_sb2st_f32 leaves them (tau2: [n][n / NB + 1 rounded up, see
 * vivit_sb2st_f32_workspace_bytes] in its workspace).  mode 0: one launch per wavefront step of reflector blocks
 * (fp32 MFMA, q2apply.hip); mode 1: one persistent launch per ~2 GB of block images, a row slab per workgroup with a
 * sliding column window, fp32 products from exact three-way bf16 splits (q2slide.hip; needs n % 4 == 0, ldz % 4 == 0,
 * 16-byte aligned Zt: VIVIT_E_UNSUPPORTED otherwise); mode -1: what vivit_symeig_f32 would pick for this shape.
 * Replaces the eigenvector half of Tensor.symeig(eigenvectors=True), vivit/linalg/eigh.py:248-250. */
size_t vivit_q2_apply_f32_workspace_bytes(int64_t n);
int vivit_q2_apply_f32(float *Zt, int64_t ldz, int64_t nrows, int64_t n, const float *R2, int64_t ldr, const float *tau2,
                       void *workspace, size_t workspace_bytes, int mode, void *stream);

/* Eigen-decomposition of a symmetric TRIDIAGONAL matrix (d: [n] diagonal, e: [n-1]
 * off-diagonal; both destroyed).  Stage 2 of vivit_symeig_f32, exported for testing. */
size_t vivit_stedc_f32_workspace_bytes(int64_t n, int want_vectors);
int vivit_stedc_f32(float *d, float *e, int64_t n, float *w, float *Z, int64_t ldz,
                    void *workspace, size_t workspace_bytes, int32_t *info, void *stream);

/* ---------------------------------------------------------------------------------------------
 * K6  Directional curvatures from the Gram eigenvectors:
 *   lambdas[n, k] = scale * sum_c ( sum_i G[(c,n), i] E[i, k] )^2 / evals[k]
 *   G: [C*N, C*N], E: [C*N, K] (ld = lde), evals: [K], lambdas: [N, K].
 *   GE: [C*N, K] scratch holding G @ E (computed by vivit_gemm_nn_f32 beforehand).
 * Replaces (V_n_T_V_e_d ** 2).sum(0) / evals
 *   vivit/optim/directional_damped_newton.py:348-351, directional_derivatives.py:322-325.
 * ------------------------------------------------------------------------------------------- */
int vivit_dir_curvature_f32(const float *GE, const float *evals, float *lambdas, int64_t C,
                            int64_t N, int64_t K, float scale, void *stream);

/* K5 epilogue / K10: out[r, k] = in[r, k] * (pre) / sqrt(evals[k])   (column scaling)
 * Replaces "/ evals.sqrt()"  vivit/optim/directional_damped_newton.py:342. */
int vivit_scale_cols_rsqrt_f32(float *X, const float *evals, int64_t rows, int64_t K, int64_t ldx,
                               float pre, void *stream);

/* ---------------------------------------------------------------------------------------------
 * K5 + K6 for `batch` per-layer groups of ONE Gram size in one launch: first- and second-order directional
 * derivatives from the kept Gram eigenvectors, without G E in memory.  Per problem b, K = K[b]:
 *   gammas[b][j, k]  = alpha_gamma * sum_i VtG[b][i, j] Zt[b][k, i] / sqrt(evals[b][k])
 *   lambdas[b][m, k] = lambda_scale * sum_c ( alpha_gram * sum_i G[b][(c, m), i] Zt[b][k, i] )^2 / evals[b][k]
 * G, Zt, evals, VtG, K, gammas, lambdas: HOST arrays of `batch` entries, read before the call returns.
 *   G[b]: DEVICE [n, n], ldg >= n, symmetric, n = C * N; read in full, not modified.
 *   Zt[b]: DEVICE [K[b]][ldz >= n], row k = unit eigenvector, as vivit_symeig_select_batched_f32 writes them.
 *   evals[b]: DEVICE [K[b]], the kept eigenvalues, already scaled.  VtG[b]: DEVICE [n, M], ldv >= M (V_t_g_n flattened).
 *   K[b]: HOST, 0 <= K[b] <= n, may differ between problems; with K[b] = 0 the problem's pointers may be NULL and
 *     nothing of it is touched.  gammas[b]: DEVICE [M, K[b]], lambdas[b]: DEVICE [N, K[b]], both contiguous.
 * Any batch >= 1 and any n >= 1; the problem index is in the grid (the descriptors travel as kernel arguments, 64 per
 * launch, so a batch of up to 64 is ONE launch).  fp32 accumulation, fixed summation order, no atomics; a problem's
 * results are bit-independent of the rest of the batch.  evals[k] <= 0 gives the IEEE class (inf / NaN) that
 * vivit_scale_cols_rsqrt_f32 and vivit_dir_curvature_f32 give.  VIVIT_E_BADARG: null array or operand, negative size,
 * C * N != n, K[b] outside 0..n, short leading dimension; nothing is launched then.
 * Replaces, per group, "V_t_g_n contracted with evecs / evals.sqrt()" and "(V_n_T_V_e_d ** 2).sum(0) / evals" of
 *   vivit/optim/directional_damped_newton.py:342,348-351 and vivit/optim/directional_derivatives.py:317,322-325 (K5/K6),
 * i.e. the four launches vivit_gemm_tn_f32 + vivit_scale_cols_rsqrt_f32 + vivit_gemm_nn_f32 + vivit_dir_curvature_f32.
 * ------------------------------------------------------------------------------------------- */
int vivit_gram_directions_batched_f32(const float *const *G, int64_t batch, int64_t n, int64_t ldg,
                                      const float *const *Zt, int64_t ldz, const float *const *evals,
                                      const float *const *VtG, int64_t ldv, const int64_t *K, int64_t C, int64_t N,
                                      int64_t M, float alpha_gram, float alpha_gamma, float lambda_scale,
                                      float *const *gammas, float *const *lambdas, void *stream);

/* K10  Squared 2-norms of K stacked vectors: acc[k] += sum_j X[k, j]^2, X: [K, len] contiguous;
 *      then vivit_scale_rows_f32 applies X[k, :] *= rsqrt(acc[k]).
 * Replaces normalize  vivit/linalg/utils.py:67-76. */
size_t vivit_row_sqnorm_workspace_bytes(int64_t K, int64_t len);
int vivit_row_sqnorm_acc_f32(const float *X, float *acc, int64_t K, int64_t len, void *workspace,
                             size_t workspace_bytes, void *stream);
int vivit_scale_rows_rsqrt_f32(float *X, const float *acc, int64_t K, int64_t len, void *stream);

/* Optional kernel timing for roofline reports (bench.py): between begin and end, every Gram SYRK
 * launch and every `symv_stride`-th symmetric matrix-vector launch of the tridiagonalisation is
 * bracketed by HIP events on its stream.  vivit_profile_end synchronises on those events and
 * fills out[6] = {syrk launches, syrk ms, syrk flops n(n+1)p,  symv launches, symv ms,
 * symv algorithmic bytes 4*m(m+1)/2}.  Not thread-safe; leave off in production. */
int vivit_profile_begin(int symv_stride);
int vivit_profile_end(double *out);
/* Per-stage time of the vivit_symeig*_f32 calls issued since vivit_profile_begin (HIP events at the stage
 * boundaries, on the launch stream), summed over calls, in ms.  out_ms[k], k < num (host pointer):
 *   1 prescale + mirror, 2 full -> band (sy2sb), 3 band -> tridiagonal (sb2st), 4 tridiagonal eigenproblem
 *   (divide & conquer | Sturm multisection | inverse iteration), 5 back-transformation Q2, 6 back-transformation
 *   Q1 / Q, 7 sort + transpose into the output, 8 one-stage tridiagonalisation (sytrd); two parts of stage 2 are
 *   reported on their own and NOT included in out_ms[2]: 9 its streaming panel products P^T = V^T A22 (fp32 MFMA),
 *   10 its delayed trailing updates (bf16 pipe).  Synchronises on the
 *   recorded events and clears them; call before vivit_profile_end or after, once. */
int vivit_profile_stages(double *out_ms, int num);

/* Mirror the lower triangle of G into the upper triangle (G[i][j] = G[j][i], i < j). */
int vivit_symmetrize_lower_f32(float *G, int64_t n, int64_t ldg, void *stream);

/* Lower triangle of a symmetric matrix <-> packed vector, packed[i (i + 1) / 2 + j] = G[i][j] (j <= i; n (n + 1) / 2 floats):
 * the partial Gram matrices of the ranks are all-reduced in this form (half the bytes of `gram += gram_p` summed over
 * ranks, vivit/utils/gram.py:104-116).  unpack writes the lower triangle and mirrors it (both triangles valid). */
int vivit_pack_lower_f32(const float *G, int64_t n, int64_t ldg, float *packed, void *stream);
int vivit_unpack_lower_f32(const float *packed, int64_t n, float *G, int64_t ldg, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* VIVIT_HIP_H */
