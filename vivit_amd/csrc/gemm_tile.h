// What the device code of more than one GEMM kernel family uses (gemm_tile128.hip, gemm_tile256.hip, gemm_tile256_bx.hip,
// gemm64.hip, gemm_tsk.hip, gemm_f32.hip): the K tile and the small tile's constants, global-address-space loads, the
// XCD-aware tile maps, the global -> LDS DMA tiles of the 256-wide kernels and the exact three-way bf16 split of a value pair.
#pragma once
#include <type_traits>

#include "common.h"

namespace vivit {

constexpr int BM = 128, BN = 128, BK = 16;     // default tile (2 x 2 waves); the WM = 1 variant is 64 x 256
constexpr int SK = BK + 4;                     // LDS row stride (floats) of a LAY_K tile [rows][20]
__host__ __device__ constexpr int tile_floats(int rows) {  // one operand tile of `rows` rows in either layout
  return rows * SK > BK * (rows + 4) ? rows * SK : BK * (rows + 4);
}
constexpr int SB = 16;                         // super-block edge in tiles

// Operand pointers are re-read from a device-resident descriptor in batched mode, which makes
// hipcc lose their address space and emit flat_load (slower, and waited for with vmcnt(0) +
// lgkmcnt(0)).  All global accesses therefore go through explicitly global-address-space pointers.
typedef const float __attribute__((address_space(1))) *gcptr;
typedef float __attribute__((address_space(1))) *gptr;
typedef const f32x4 __attribute__((address_space(1))) *gcptr4;
__device__ __forceinline__ float4 ldg4(gcptr q) {
  const f32x4 v = *(gcptr4)q;
  return make_float4(v.x, v.y, v.z, v.w);
}

// Guarded element load, BRANCH-FREE: out-of-range elements read a clamped in-range address and
// select zero.  (A branch per load makes hipcc put s_waitcnt vmcnt(0) in front of every load and
// in front of the MFMA block, which serialises the stream and exposes the full HBM latency.)
__device__ __forceinline__ float ld1_sel(gcptr P, int64_t idx_major, int64_t n_major,
                                         int64_t idx_minor, int64_t n_minor, int64_t ld) {
  const bool ok = idx_major < n_major && idx_minor < n_minor;
  const int64_t a = idx_major < n_major ? idx_major : n_major - 1;
  const int64_t b = idx_minor < n_minor ? idx_minor : n_minor - 1;
  const float x = P[a * ld + b];
  return ok ? x : 0.f;
}

// Super-block geometry: 256 tiles per super-block, SBH x SBW tiles (16 x 16 for large outputs; for
// skinny outputs the short side shrinks to the next power of two >= its tile count, so that a
// one-tile-wide or one-tile-tall GEMM still spreads over all 8 XCDs), each XCD owning one compact
// sub-block of 32 tiles (xh x xw).
__host__ __device__ inline int sb_width(int tiles_m, int tiles_n) {
  int w = 1;
  while (w < 16 && w < tiles_n) w <<= 1;
  if (w == 16 && tiles_m < 16) {  // short in M instead: widen the super-block
    int hgt = 1;
    while (hgt < 16 && hgt < tiles_m) hgt <<= 1;
    w = 256 / hgt;
  }
  return w;
}

// blockIdx.x -> (tile_i, tile_j); returns false for padding slots.
__device__ __forceinline__ bool map_tile(int syrk, int SBW, int tiles_m, int tiles_n, int &ti, int &tj) {
  const int sb = blockIdx.x >> 8;
  // split-K: rotate the slots with the split index.  Workgroups go to XCD (linear id % 8) and every split's
  // grid row starts at a multiple of 256, so without the rotation slot 0 of EVERY split - the only valid one of
  // a single-tile output - lands on XCD 0 and the whole product runs on one eighth of the chip.
  const int slot = (blockIdx.x - blockIdx.y) & 255;
  const int SBH = 256 / SBW;
  int I, J;
  if (syrk) {
    I = (int)((sqrtf(8.f * (float)sb + 1.f) - 1.f) * 0.5f);
    while ((I + 1) * (I + 2) / 2 <= sb) ++I;
    while (I * (I + 1) / 2 > sb) --I;
    // row I of the super-block triangle from its diagonal block leftwards: the LAST super-block of the grid is then an
    // off-diagonal one (diagonal tiles flush their accumulators more often - bx_flush_tiles - and a slower tail block
    // delayed every chunk launch of the Gram SYRK)
    J = I - (sb - I * (I + 1) / 2);
  } else {
    const int sbn = (tiles_n + SBW - 1) / SBW;
    I = sb / sbn;
    J = sb - I * sbn;
  }
  const int xcd = slot & 7, w = slot >> 3;
  // Workgroups are dealt round-robin to the 8 XCDs (blockIdx % 8), so every super-block must hand each XCD
  // the same number of tiles or the busiest XCD sets the kernel time.  Full rectangular super-blocks do
  // (32 tiles per XCD in a compact sub-block).  The others - the lower triangles on the diagonal of a SYRK
  // and the partial super-blocks at the bottom/right edge - are dealt out evenly instead: XCD x takes the
  // c = ceil(v / 8) consecutive valid tiles [c x, c x + c) in row-major order.  (Config-2 Gram matrix before
  // this: 26/10/0/0/32/32/26/10 tiles of every diagonal super-block per XCD, busiest XCD 1760 tiles against
  // a mean of 1610, kernel 9 % over its MFMA time.)
  const int vr = tiles_m - I * SBH < SBH ? tiles_m - I * SBH : SBH;  // valid rows / columns of this super-block
  const int vc = tiles_n - J * SBW < SBW ? tiles_n - J * SBW : SBW;
  if (syrk && I == J) {
    const int d = vr < vc ? vr : vc;  // triangle edge
    const int v = d * (d + 1) / 2, c = (v + 7) >> 3;
    const int idx = c * xcd + w;
    if (w >= c || idx >= v) return false;
    int a = (int)((sqrtf(8.f * (float)idx + 1.f) - 1.f) * 0.5f);
    while ((a + 1) * (a + 2) / 2 <= idx) ++a;
    while (a * (a + 1) / 2 > idx) --a;
    ti = I * SBH + a;
    tj = J * SBW + (idx - a * (a + 1) / 2);
    return true;
  }
  if (vr < SBH || vc < SBW) {
    if (vr <= 0 || vc <= 0) return false;
    const int v = vr * vc, c = (v + 7) >> 3;
    const int idx = c * xcd + w;
    if (w >= c || idx >= v) return false;
    ti = I * SBH + idx / vc;
    tj = J * SBW + idx % vc;
    return true;
  }
  int xw = SBW < 4 ? SBW : 4, xh = 32 / xw;          // XCD sub-block: xh x xw tiles
  if (xh > SBH) { xh = SBH; xw = 32 / xh; }
  const int xcols = SBW / xw;                         // XCD sub-blocks per super-block row
  ti = I * SBH + (xcd / xcols) * xh + w / xw;
  tj = J * SBW + (xcd % xcols) * xw + w % xw;
  if (ti >= tiles_m || tj >= tiles_n) return false;
  if (syrk && tj > ti) return false;
  return true;
}

// map_tile + the K split of the workgroup.  SBW >= 0: the split is blockIdx.y.  SBW < 0 (the split-K launches of SMALL outputs: one
// partial super-block of v valid tiles): a COMPACT one-dimensional grid of 8 v ceil(nsplit / 8) workgroups, workgroup L -> tile
// (L / 8) % v of split 8 (L / 8 / v) + L % 8.  Workgroups go to XCD L % 8, so ALL tiles of a split run on ONE XCD at about the same
// time and share their operand panels in its L2 -- the padded grid (256 slots per split row, slots rotated over the XCDs) gave
// every XCD tiles of many splits that share nothing, so the product ran at the HBM rate of 48 KB per K tile and workgroup, and its
// 8 200 padding workgroups (each asking for a whole CU's LDS) queued for whatever CU was free: the config-1 Gram SYRK (n = 1280,
// K = 401 408: 15 tiles x 34 splits) took 7.1 ms for 2.4 ms of tile time (profiles/r06_splitk_compact.log).
__device__ __forceinline__ bool map_tile_z(int syrk, int SBW, int tiles_m, int tiles_n, int nsplit, int &ti, int &tj, int &zsplit) {
  if (SBW >= 0) {
    zsplit = (int)blockIdx.y;
    return map_tile(syrk, SBW, tiles_m, tiles_n, ti, tj);
  }
  const int d = tiles_m < tiles_n ? tiles_m : tiles_n;
  const int v = syrk ? d * (d + 1) / 2 : tiles_m * tiles_n;
  const int L = (int)blockIdx.x, r = L >> 3;
  const int idx = r % v;
  zsplit = 8 * (r / v) + (L & 7);
  if (zsplit >= nsplit) return false;
  if (syrk) {
    int a = (int)((sqrtf(8.f * (float)idx + 1.f) - 1.f) * 0.5f);
    while ((a + 1) * (a + 2) / 2 <= idx) ++a;
    while (a * (a + 1) / 2 > idx) --a;
    ti = a;
    tj = idx - a * (a + 1) / 2;
  } else {
    ti = idx / tiles_n;
    tj = idx % tiles_n;
  }
  return true;
}

// ---- the DMA-fed tiles (gemm256_kernel; the 64-row streaming kernels take the loaders with their own ROWS)
constexpr int B2 = 256;

template <int LAY, int ROWS = B2>
__device__ __forceinline__ void frag_half(const float *__restrict__ s, int row, int q, int h, float (&fr)[4]) {
  if (LAY == LAY_K) {
    const int c = (2 * q + h) ^ ((row >> 2) & 3);
    const float4 v = *reinterpret_cast<const float4 *>(s + row * BK + 4 * c);
    fr[0] = v.x; fr[1] = v.y; fr[2] = v.z; fr[3] = v.w;
  } else {
#pragma unroll
    for (int t = 0; t < 4; ++t) fr[t] = s[(8 * q + 4 * h + t) * ROWS + row];
  }
}

// this lane's global source for 1 KB block `blk` (0..15) of an operand tile at K offset 0
template <int LAY, int ROWS = B2>
__device__ __forceinline__ gcptr dma_src(const float *P, int64_t ld, int64_t row0, int64_t nrows, int blk, int lane) {
  if (LAY == LAY_K) {  // block = 16 rows x 16 k; lane -> (row, swizzled 16-byte chunk)
    const int rl = lane >> 2, pos = lane & 3;
    int64_t row = row0 + 16 * blk + rl;
    row = row < nrows ? row : nrows - 1;
    return (gcptr)(P + row * ld + 4 * (pos ^ ((rl >> 2) & 3)));
  } else {             // tile [16 k][ROWS]; block = its floats [256 blk, 256 blk + 256); lane -> 4 of them
    const int f = 256 * blk + 4 * lane, kr = f / ROWS;
    int64_t row = row0 + (f - kr * ROWS);
    row = row + 4 <= nrows ? row : nrows - 4;  // nrows % 4 == 0 and nrows >= 4 (host)
    return (gcptr)(P + (int64_t)kr * ld + row);
  }
}

__device__ __forceinline__ void dma16(gcptr src, unsigned lds_byte_addr) {
  __asm__ volatile("s_mov_b32 m0, %0\n\tglobal_load_lds_dwordx4 %1, off" ::"s"(lds_byte_addr), "v"(src) : "memory");
}

// ---- the bf16 pipe: exact three-way split of two fp32 values (see gemm_tile256_bx.hip)
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ void bx_split2(float a, float b, unsigned &hi, unsigned &mid, unsigned &lo) {
  const bf16x2 h = {(__bf16)a, (__bf16)b};
  hi = __builtin_bit_cast(unsigned, h);
  const float ra = a - __uint_as_float(hi << 16), rb = b - __uint_as_float(hi & 0xffff0000u);
  const bf16x2 m = {(__bf16)ra, (__bf16)rb};
  mid = __builtin_bit_cast(unsigned, m);
  const float sa = ra - __uint_as_float(mid << 16), sb = rb - __uint_as_float(mid & 0xffff0000u);
  const bf16x2 l = {(__bf16)sa, (__bf16)sb};
  lo = __builtin_bit_cast(unsigned, l);
}

} // namespace vivit
