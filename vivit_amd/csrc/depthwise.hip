// Depthwise convolution (groups = C, Cout = C mult, zero padding): the input rule and the weight rule of Conv1d / Conv2d layers
// whose every channel has its own filter (ConvNeXt's 7 x 7 token mixer, the 3 x 3 / 5 x 5 layers of MobileNet and EfficientNet,
// the causal Conv1d in front of a Mamba block).  vivit_dwconv2d_jac_t_f32 and vivit_dwconv2d_weight_mjp_f32 (include/vivit_hip.h),
// ONE launch each, no workspace, no atomics.  A depthwise convolution has NO channel contraction: per plane it is a stencil (input
// rule) or KH KW correlations of two planes (weight rule), bound by memory and by the LDS, never by the arithmetic.  There is no
// matrix product to hand to the MFMA pipe -- the "GEMM" of a plane would be 1 x KH KW x OH OW with a gathered operand -- so both
// kernels are plain FMA code on LDS-resident operands; do not try MFMA here.
//
// INPUT RULE  out[r, c, h, w] = sum_j sum_{a, b} M[r, c mult + j, oh, ow] weight[c mult + j, 0, a, b],  oh sh - ph + a dh = h,
// ow sw - pw + b dw = w.  dwconv2d_jac_t_kernel<FAST>, 256 lanes.  A lane owns FOUR consecutive w of one row h of one (r, c) plane and
// writes them with one 16-byte store when W % 4 == 0 (scalar stores otherwise).  A workgroup owns a tile of th rows x 4 gw columns of
// a plane (gw th <= 256; gw <= 16 groups, or <= 256 groups = DWJ_ROW_TILE columns for the one-row image of a Conv1d, which so tiles
// along W), or, when the whole plane is one tile, the floor(256 / (gw th)) consecutive planes that fill its lanes (a 7 x 7 plane:
// 18 planes, 252 lanes; 14 x 14: 4 planes, 224 lanes).  Per channel-multiplier index j it stages, per plane, the KH KW filter values
// and the patch of M[r, c mult + j] its tile can reach -- rows oh_b .. oh_b + PH - 1 with oh_b = floor((h0 + ph - (KH - 1) dh) / sh),
// likewise the columns; zero outside [0, OH) x [0, OW) -- and then gathers from LDS only.  A stride > 1 is handled in the gather:
// a tap contributes where h + ph - a dh is a multiple of sh (M is never zero-inserted in memory); FAST is sh = sw = dw = 1, where
// the four outputs of a lane slide a four-word window over the patch row (one LDS read per tap instead of four).
// SUMMATION ORDER of an output element: j ascending, a ascending, b DESCENDING, each term added by one fmaf to a sum that starts at
// +0; taps the stride excludes are skipped (a position no window reads stays +0).  Every element of out has exactly one writer.
//
// WEIGHT RULE  V[r, cm, 0, a, b] = sum_{oh, ow} M[r, cm, oh, ow] x[r % N, cm / mult, oh sh - ph + a dh, ow sw - pw + b dw].
// dwconv2d_weight_mjp_kernel<NCH>, 256 lanes.  A workgroup owns whole (r, cm) planes: one, all 256 lanes on it, or -- planes of at most
// 128 positions -- four, one per wave.  It walks the plane of M in tiles of SR rows x SC columns, row-major (the whole plane when M and
// the x patch fit the LDS; else as many whole rows as fit; a single row that does not fit is cut along OW: the long Conv1d), staging
// the M tile and the x patch it reads, ZERO-BORDERED (the gather has no bounds test).  A lane owns the positions lane, lane + LP,
// lane + 2 LP .. of the tile (LP = 256 or 64 lanes per plane) and keeps one partial sum per tap IN REGISTERS across all tiles of the
// plane: 16 NCH accumulators, NCH = ceil(KH KW / 16) rounded up to 1, 2, 4 or 8.  The taps are processed in chunks of 16 over the
// resident tile (16 uniform LDS offsets per chunk; M is re-read once per chunk).
// SUMMATION ORDER of V[r, cm, a, b]: per lane its positions ascending, tiles row-major, fmaf onto +0; then the 64 lanes of a wave by
// the fixed fold dw_wave_fold (xor 32, 16, 8, 4 while halving the 16 taps of a chunk between the partners, then xor 2, 1); then the
// waves of the plane in ascending order.  The plan (SR, SC, planes per workgroup) is a function of the geometry alone, so the bytes of
// a result depend on the arguments and the data only.
//
// Both grids are capped at DW_GRID_CAP workgroups (eight per compute unit at full occupancy) and looped over; plane and row offsets
// are 64-bit, offsets inside a plane 32-bit (a plane of 2^31 elements or more is VIVIT_E_UNSUPPORTED).  Both kernels stay within the
// default 64 KB of dynamic LDS (DW_LDS_FLOATS), as attention_forward.hip does.  (vivit_amd/kernels.py repeats DW_LDS_FLOATS,
// DW_RED_FLOATS, DWJ_ROW_TILE and the lane count for the tests that place a plane one row past a tile: change them together.)
#include "common.h"

namespace vivit {

constexpr int DW_THREADS = 256;
constexpr int DW_GRID_CAP = 2048;                  // workgroups of a launch (<= the 32768 of the other rule kernels)
constexpr int DW_LDS_FLOATS = 16384;               // 64 KB: the default dynamic-LDS limit
constexpr int DW_MAX_TAPS = 128;
constexpr int DWJ_ROW_TILE = 1024;                 // columns of an input-rule tile of a one-row image
constexpr int DW_RED_FLOATS = 4 * DW_MAX_TAPS;     // weight rule: the waves' folded sums [wave][tap]
static_assert(DW_GRID_CAP <= 32768 && DW_LDS_FLOATS * 4 <= 64 * 1024, "grid cap and default dynamic LDS limit");

struct DwGeom {
  int C, mult, H, W, KH, KW, OH, OW, sh, sw, ph, pw, dh, dw;
};

struct DwJtPlan {   // input rule
  int gw, th;             // tile: th rows of gw groups of four columns
  int tiles_h, tiles_w;   // tiles of a plane
  int ppw;                // planes per workgroup (> 1 only when the plane is one tile)
  int PH, PW;             // rows / columns of the staged patch of M
  int64_t units;          // work items of the launch: (plane, tile), or groups of ppw planes
};

struct DwWPlan {    // weight rule
  int SR, SC;             // tile of M
  int XR, XC;             // zero-bordered patch of x a full tile reads
  int ppw;                // planes per workgroup: 1 (256 lanes per plane) or 4 (one wave per plane)
  int region;             // LDS floats of one plane's tile + patch
  int64_t units;
};

__host__ __device__ inline int dw_floordiv(int a, int b) { return a >= 0 ? a / b : -((-a + b - 1) / b); }

template <bool FAST>
__global__ __launch_bounds__(DW_THREADS) void dwconv2d_jac_t_kernel(const float *__restrict__ M, const float *__restrict__ Wt,
                                                                    float *__restrict__ out, DwGeom g, DwJtPlan p, int64_t planes,
                                                                    int vec) {
  extern __shared__ __attribute__((aligned(16))) float dw_smem[];
  const int KK = g.KH * g.KW, PP = p.PH * p.PW;
  float *sF = dw_smem;                 // [ppw][KK]  filters of the planes' channels, index j
  float *sP = dw_smem + p.ppw * KK;    // [ppw][PH][PW]  patches of M
  const int tid = threadIdx.x, lpp = p.gw * p.th;
  const int slot = tid / lpp, rem = tid - slot * lpp, lr = rem / p.gw, lc = rem - lr * p.gw;
  const int tpp = p.tiles_h * p.tiles_w;
  const int64_t msz = (int64_t)g.OH * g.OW, osz = (int64_t)g.H * g.W;
  for (int64_t u = blockIdx.x; u < p.units; u += gridDim.x) {
    int64_t plane0;
    int h0 = 0, w0 = 0;
    if (tpp == 1) {
      plane0 = u * p.ppw;
    } else {
      plane0 = u / tpp;
      const int t = (int)(u - plane0 * tpp), ty = t / p.tiles_w;
      h0 = ty * p.th;
      w0 = (t - ty * p.tiles_w) * p.gw * 4;
    }
    const int ohb = dw_floordiv(h0 + g.ph - (g.KH - 1) * g.dh, g.sh), owb = dw_floordiv(w0 + g.pw - (g.KW - 1) * g.dw, g.sw);
    const int h = h0 + lr, w = w0 + 4 * lc;
    const bool active = slot < p.ppw && plane0 + slot < planes && h < g.H && w < g.W;
    float acc[4] = {0.f, 0.f, 0.f, 0.f};
    for (int j = 0; j < g.mult; ++j) {
      __syncthreads();   // the previous j (or work item) has been read
      for (int idx = tid; idx < p.ppw * KK; idx += DW_THREADS) {
        const int s = idx / KK, e = idx - s * KK;
        const int64_t P = plane0 + s;
        sF[idx] = P < planes ? Wt[((P % g.C) * g.mult + j) * KK + e] : 0.f;
      }
      for (int idx = tid; idx < p.ppw * PP; idx += DW_THREADS) {
        const int s = idx / PP, e = idx - s * PP, pr = e / p.PW, pc = e - pr * p.PW;
        const int oh = ohb + pr, ow = owb + pc;
        const int64_t P = plane0 + s;
        float v = 0.f;
        if (P < planes && oh >= 0 && oh < g.OH && ow >= 0 && ow < g.OW) v = M[(P * g.mult + j) * msz + (int64_t)oh * g.OW + ow];
        sP[idx] = v;
      }
      __syncthreads();
      if (active) {
        const float *f = sF + slot * KK, *pt = sP + slot * PP;
        if (FAST) {   // sh = sw = dw = 1: owb = w0 + pw - (KW - 1), the window of tap b = KW - 1 starts at column w - w0
          for (int a = 0; a < g.KH; ++a) {
            const float *row = pt + (h + g.ph - a * g.dh - ohb) * p.PW + (w - w0);
            float v0 = row[0], v1 = row[1], v2 = row[2], v3 = row[3];
            for (int b = g.KW - 1; b >= 0; --b) {
              const float fw = f[a * g.KW + b];
              acc[0] = fmaf(v0, fw, acc[0]);
              acc[1] = fmaf(v1, fw, acc[1]);
              acc[2] = fmaf(v2, fw, acc[2]);
              acc[3] = fmaf(v3, fw, acc[3]);
              if (b > 0) {
                v0 = v1; v1 = v2; v2 = v3;
                v3 = row[g.KW - b + 3];
              }
            }
          }
        } else {
          for (int a = 0; a < g.KH; ++a) {
            const int t = h + g.ph - a * g.dh - ohb * g.sh;   // >= 0
            if (t % g.sh) continue;
            const float *row = pt + (t / g.sh) * p.PW;
            for (int b = g.KW - 1; b >= 0; --b) {
              const float fw = f[a * g.KW + b];
              const int c0 = w + g.pw - b * g.dw - owb * g.sw;   // >= 0
#pragma unroll
              for (int q = 0; q < 4; ++q)
                if ((c0 + q) % g.sw == 0) acc[q] = fmaf(row[(c0 + q) / g.sw], fw, acc[q]);
            }
          }
        }
      }
    }
    if (active) {
      float *o = out + (plane0 + slot) * osz + (int64_t)h * g.W + w;
      if (vec) {
        *reinterpret_cast<float4 *>(o) = make_float4(acc[0], acc[1], acc[2], acc[3]);
      } else {
#pragma unroll
        for (int q = 0; q < 4; ++q)
          if (w + q < g.W) o[q] = acc[q];
      }
    }
  }
}

// The sums of 16 taps over the 64 lanes of a wave, a fixed tree: at xor 32, 16, 8, 4 the partners split the taps they still hold
// (the lane with the bit set keeps the upper half and sends the lower), at xor 2 and 1 they add the one that is left.  Afterwards
// v[0] of every lane is the wave's sum of tap (lane >> 2) & 15.  17 exchanges instead of 96.
__device__ inline void dw_wave_fold(float (&v)[16], int lane) {
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

template <int NCH>
__global__ __launch_bounds__(DW_THREADS) void dwconv2d_weight_mjp_kernel(const float *__restrict__ M, const float *__restrict__ x,
                                                                         float *__restrict__ V, DwGeom g, DwWPlan p, int64_t planes,
                                                                         int64_t N) {
  extern __shared__ __attribute__((aligned(16))) float dw_smem[];
  const int KK = g.KH * g.KW, CM = g.C * g.mult;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int LP = DW_THREADS / p.ppw, wps = 4 / p.ppw;   // lanes and waves of a plane
  const int slot = tid / LP, lg = tid - slot * LP;
  float *sRed = dw_smem;                                      // [wave][DW_MAX_TAPS]
  float *sM = dw_smem + DW_RED_FLOATS + slot * p.region;     // [SR][SC]
  float *sX = sM + p.SR * p.SC;                               // [XR][XC]
  const int64_t msz = (int64_t)g.OH * g.OW, xsz = (int64_t)g.H * g.W;
  for (int64_t u = blockIdx.x; u < p.units; u += gridDim.x) {
    const int64_t Q = u * p.ppw + slot;
    const bool live = Q < planes;
    const int64_t r = live ? Q / CM : 0;
    const int cm = live ? (int)(Q - r * CM) : 0;
    const float *Mp = M + (live ? Q : 0) * msz;
    const float *xp = x + ((r % N) * g.C + cm / g.mult) * xsz;
    float acc[NCH][16];
#pragma unroll
    for (int ch = 0; ch < NCH; ++ch)
#pragma unroll
      for (int t = 0; t < 16; ++t) acc[ch][t] = 0.f;
    for (int oh0 = 0; oh0 < g.OH; oh0 += p.SR) {
      for (int ow0 = 0; ow0 < g.OW; ow0 += p.SC) {
        const int vr = g.OH - oh0 < p.SR ? g.OH - oh0 : p.SR, vc = g.OW - ow0 < p.SC ? g.OW - ow0 : p.SC;
        const int xr = (vr - 1) * g.sh + (g.KH - 1) * g.dh + 1, xc = (vc - 1) * g.sw + (g.KW - 1) * g.dw + 1;
        const int npos = vr * vc;
        __syncthreads();   // the previous tile has been read
        if (live) {
          for (int idx = lg; idx < npos; idx += LP) {
            const int rr = idx / vc, cc = idx - rr * vc;
            sM[rr * p.SC + cc] = Mp[(int64_t)(oh0 + rr) * g.OW + ow0 + cc];
          }
          const int ih0 = oh0 * g.sh - g.ph, iw0 = ow0 * g.sw - g.pw;
          for (int idx = lg; idx < xr * xc; idx += LP) {
            const int rr = idx / xc, cc = idx - rr * xc;
            const int ih = ih0 + rr, iw = iw0 + cc;
            sX[rr * p.XC + cc] = (ih >= 0 && ih < g.H && iw >= 0 && iw < g.W) ? xp[(int64_t)ih * g.W + iw] : 0.f;
          }
        }
        __syncthreads();
        if (live && lg < npos) {
          const int lr0 = lg / vc, lc0 = lg - lr0 * vc, dq = LP / vc, dr = LP - dq * vc;
#pragma unroll
          for (int ch = 0; ch < NCH; ++ch) {
            if (ch * 16 < KK) {
              int toff[16];   // uniform: offset of the tap's operand from that of tap (0, 0); a tap >= KK reads tap (0, 0), its sum is dropped
#pragma unroll
              for (int t = 0; t < 16; ++t) {
                const int tap = ch * 16 + t, a = tap / g.KW, b = tap - a * g.KW;
                toff[t] = tap < KK ? a * g.dh * p.XC + b * g.dw : 0;
              }
              int lr = lr0, lc = lc0;
              for (int pos = lg; pos < npos; pos += LP) {
                const float m = sM[lr * p.SC + lc];
                const float *xb = sX + lr * g.sh * p.XC + lc * g.sw;
#pragma unroll
                for (int t = 0; t < 16; ++t) acc[ch][t] = fmaf(m, xb[toff[t]], acc[ch][t]);
                lc += dr;
                lr += dq;
                if (lc >= vc) { lc -= vc; ++lr; }
              }
            }
          }
        }
      }
    }
    // (sRed was last read before the barriers of this work item's tiles: OH, OW >= 1, so there was at least one tile)
#pragma unroll
    for (int ch = 0; ch < NCH; ++ch) {
      if (ch * 16 < KK) {   // (uniform)
        dw_wave_fold(acc[ch], lane);
        if ((lane & 3) == 0) sRed[wave * DW_MAX_TAPS + ch * 16 + (lane >> 2)] = acc[ch][0];
      }
    }
    __syncthreads();
    for (int idx = tid; idx < p.ppw * KK; idx += DW_THREADS) {
      const int s = idx / KK, t = idx - s * KK;
      const int64_t Qs = u * p.ppw + s;
      if (Qs < planes) {
        float sum = sRed[(s * wps) * DW_MAX_TAPS + t];
        for (int wv = 1; wv < wps; ++wv) sum += sRed[(s * wps + wv) * DW_MAX_TAPS + t];
        V[Qs * KK + t] = sum;
      }
    }
  }
}

// ---- host: checks and plans -------------------------------------------------------------------------------------------------------
// The checks both entry points share; fills g when the status is VIVIT_OK.
static int dw_check(int64_t rows, int64_t C, int64_t mult, int64_t H, int64_t W, int64_t KH, int64_t KW, int64_t OH, int64_t OW, int64_t sh,
                    int64_t sw, int64_t ph, int64_t pw, int64_t dh, int64_t dw, DwGeom *g) {
  if (rows < 0 || C <= 0 || mult <= 0 || H <= 0 || W <= 0 || KH <= 0 || KW <= 0 || OH <= 0 || OW <= 0 || sh <= 0 || sw <= 0 || ph < 0 ||
      pw < 0 || dh <= 0 || dw <= 0)
    return VIVIT_E_BADARG;
  const int64_t lim = 1LL << 30;   // every size fits an int and the products below fit 64 bits
  if (rows > lim || C > lim || mult > lim || H > lim || W > lim || KH > lim || KW > lim || OH > lim || OW > lim || sh > lim || sw > lim ||
      ph > lim || pw > lim || dh > lim || dw > lim)
    return VIVIT_E_UNSUPPORTED;
  // the geometry must be that of a convolution: every output position reads inside the padded input
  if ((OH - 1) * sh + (KH - 1) * dh - ph >= H + ph || (OW - 1) * sw + (KW - 1) * dw - pw >= W + pw) return VIVIT_E_BADARG;
  if (KH * KW > DW_MAX_TAPS || H * W > 0x7fffffffLL || OH * OW > 0x7fffffffLL || C * mult > 0x7fffffffLL) return VIVIT_E_UNSUPPORTED;
  // (the halo a tile needs: beyond this no tile fits the LDS, and the index arithmetic of a tile stays far inside an int)
  if ((KH - 1) * dh >= DW_LDS_FLOATS || (KW - 1) * dw >= DW_LDS_FLOATS || sh >= DW_LDS_FLOATS || sw >= DW_LDS_FLOATS || ph > lim / 2 ||
      pw > lim / 2)
    return VIVIT_E_UNSUPPORTED;
  const int64_t big = H * W > OH * OW ? H * W : OH * OW;
  if (rows > 0 && C * mult > (1LL << 62) / big / rows) return VIVIT_E_UNSUPPORTED;   // element offsets fit 64 bits
  *g = DwGeom{(int)C, (int)mult, (int)H, (int)W, (int)KH, (int)KW, (int)OH, (int)OW, (int)sh, (int)sw, (int)ph, (int)pw, (int)dh, (int)dw};
  return VIVIT_OK;
}

// Patch extent of `n` consecutive outputs behind a halo `halo` at stride `s`: floor((lo + n - 1 + halo') / s) - floor(lo / s) + 1 over all lo
static int64_t dw_patch(int64_t n, int64_t halo, int64_t s) { return (n - 1 + halo) / s + (s > 1 ? 2 : 1); }

static bool dw_jac_t_plan(const DwGeom &g, int64_t planes, DwJtPlan *p) {
  const int64_t KK = (int64_t)g.KH * g.KW, gw_full = cdiv(g.W, 4);
  int64_t gw = gw_full < (g.H == 1 ? DWJ_ROW_TILE / 4 : 16) ? gw_full : (g.H == 1 ? DWJ_ROW_TILE / 4 : 16);
  int64_t th = g.H < DW_THREADS / gw ? g.H : DW_THREADS / gw;
  for (;;) {
    const int64_t PH = dw_patch(th, (int64_t)(g.KH - 1) * g.dh, g.sh), PW = dw_patch(4 * gw, (int64_t)(g.KW - 1) * g.dw, g.sw);
    const int64_t per = KK + PH * PW;
    if (per <= DW_LDS_FLOATS) {
      const int64_t tiles_h = cdiv(g.H, th), tiles_w = cdiv(gw_full, gw);
      int64_t ppw = 1;
      if (tiles_h * tiles_w == 1) {
        ppw = DW_THREADS / (gw * th);
        if (ppw > DW_LDS_FLOATS / per) ppw = DW_LDS_FLOATS / per;
      }
      *p = DwJtPlan{(int)gw, (int)th, (int)tiles_h, (int)tiles_w, (int)ppw, (int)PH, (int)PW,
                    ppw > 1 ? cdiv(planes, ppw) : planes * tiles_h * tiles_w};
      return true;
    }
    if (th > 1) th = (th + 1) / 2;
    else if (gw > 1) gw = (gw + 1) / 2;
    else return false;
  }
}

static bool dw_weight_plan(const DwGeom &g, int64_t planes, DwWPlan *p) {
  const int64_t hh = (int64_t)(g.KH - 1) * g.dh + 1, hw = (int64_t)(g.KW - 1) * g.dw + 1;   // patch of a single position
  const int64_t budget = DW_LDS_FLOATS - DW_RED_FLOATS;
  const int64_t xr_all = (int64_t)(g.OH - 1) * g.sh + hh, xc_all = (int64_t)(g.OW - 1) * g.sw + hw;   // patch of the whole plane
  const int64_t whole = xr_all <= budget && xc_all <= budget ? (int64_t)g.OH * g.OW + xr_all * xc_all : budget + 1;
  int64_t SR = g.OH, SC = g.OW, ppw = 1;
  if ((int64_t)g.OH * g.OW <= 128 && whole <= budget / 4) {
    ppw = 4;
  } else if (whole > budget) {
    SR = (budget - (hh - g.sh) * xc_all) / (g.OW + g.sh * xc_all);   // SR OW + ((SR - 1) sh + hh) XC <= budget
    if (SR > g.OH) SR = g.OH;
    if (SR < 1) {   // not even one row: cut it, SC + hh ((SC - 1) sw + hw) <= budget
      SR = 1;
      SC = (budget - hh * (hw - g.sw)) / (1 + hh * g.sw);
      if (SC > g.OW) SC = g.OW;
      if (SC < 1) return false;
    }
  }
  const int64_t XR = (SR - 1) * g.sh + hh, XC = (SC - 1) * g.sw + hw;
  *p = DwWPlan{(int)SR, (int)SC, (int)XR, (int)XC, (int)ppw, (int)(SR * SC + XR * XC), cdiv(planes, ppw)};
  return true;
}

} // namespace vivit

using namespace vivit;

extern "C" {

int vivit_dwconv2d_jac_t_f32(const float *M, const float *weight, float *out, int64_t rows, int64_t C, int64_t mult, int64_t H,
                             int64_t W, int64_t KH, int64_t KW, int64_t OH, int64_t OW, int64_t sh, int64_t sw, int64_t ph,
                             int64_t pw, int64_t dh, int64_t dw, void *stream) {
  DwGeom g;
  const int st = dw_check(rows, C, mult, H, W, KH, KW, OH, OW, sh, sw, ph, pw, dh, dw, &g);
  if (st != VIVIT_OK) return st;
  if (rows == 0) return VIVIT_OK;
  if (!M || !weight || !out) return VIVIT_E_BADARG;
  const int64_t planes = rows * C;
  DwJtPlan p;
  if (!dw_jac_t_plan(g, planes, &p)) return VIVIT_E_UNSUPPORTED;
  const size_t lds = sizeof(float) * (size_t)p.ppw * ((size_t)g.KH * g.KW + (size_t)p.PH * p.PW);
  const unsigned grid = (unsigned)(p.units < DW_GRID_CAP ? p.units : DW_GRID_CAP);
  const int vec = (W % 4 == 0) && (reinterpret_cast<uintptr_t>(out) & 15) == 0;
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (sh == 1 && sw == 1 && dw == 1)
    dwconv2d_jac_t_kernel<true><<<grid, DW_THREADS, lds, s>>>(M, weight, out, g, p, planes, vec);
  else
    dwconv2d_jac_t_kernel<false><<<grid, DW_THREADS, lds, s>>>(M, weight, out, g, p, planes, vec);
  return launch_status();
}

int vivit_dwconv2d_weight_mjp_f32(const float *M, const float *x, float *V, int64_t rows, int64_t N, int64_t C, int64_t mult,
                                  int64_t H, int64_t W, int64_t KH, int64_t KW, int64_t OH, int64_t OW, int64_t sh, int64_t sw,
                                  int64_t ph, int64_t pw, int64_t dh, int64_t dw, void *stream) {
  if (N <= 0) return VIVIT_E_BADARG;
  DwGeom g;
  const int st = dw_check(rows, C, mult, H, W, KH, KW, OH, OW, sh, sw, ph, pw, dh, dw, &g);
  if (st != VIVIT_OK) return st;
  if (N > (1LL << 30)) return VIVIT_E_UNSUPPORTED;
  if (rows == 0) return VIVIT_OK;
  if (!M || !x || !V) return VIVIT_E_BADARG;
  const int64_t planes = rows * C * mult;
  DwWPlan p;
  if (!dw_weight_plan(g, planes, &p)) return VIVIT_E_UNSUPPORTED;
  const size_t lds = sizeof(float) * ((size_t)DW_RED_FLOATS + (size_t)p.ppw * p.region);
  const unsigned grid = (unsigned)(p.units < DW_GRID_CAP ? p.units : DW_GRID_CAP);
  hipStream_t s = static_cast<hipStream_t>(stream);
  const int taps = g.KH * g.KW;
  if (taps <= 16) dwconv2d_weight_mjp_kernel<1><<<grid, DW_THREADS, lds, s>>>(M, x, V, g, p, planes, N);
  else if (taps <= 32) dwconv2d_weight_mjp_kernel<2><<<grid, DW_THREADS, lds, s>>>(M, x, V, g, p, planes, N);
  else if (taps <= 64) dwconv2d_weight_mjp_kernel<4><<<grid, DW_THREADS, lds, s>>>(M, x, V, g, p, planes, N);
  else dwconv2d_weight_mjp_kernel<8><<<grid, DW_THREADS, lds, s>>>(M, x, V, g, p, planes, N);
  return launch_status();
}

} // extern "C"
