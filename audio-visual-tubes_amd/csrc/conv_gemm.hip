// Implicit-GEMM convolution for the ResNet-18 trunks (fwd, dgrad, wgrad) on gfx950 MFMA.
//
// Replaces the implicit cuDNN/MKLDNN Conv2d of models/base_models.py:23-30 (conv3x3/conv1x1),
// :135-138 (7x7/s2 stems) as called from BasicBlock.forward (:53-69) and _forward_impl (:195-210).
//
// Layout: activations NHWC bf16; weights packed bf16.  fp32 accumulate in MFMA AGPRs.
//   fwd   : C[m = (n,p,q)][k_out]      = sum_{(r,s,c)}  X[n, p*st-pad+r, q*st-pad+s, c] * W[k_out][(r,s,c)]
//   dgrad : C[m = (n,h,w)][c]          = sum_{(r,s,k)}  DY[n, (h+pad-r)/st, (w+pad-s)/st, k] * WT[c][(r,s,k)]
//   wgrad : DW[k_out][(r,s,c)]        += sum_{(n,p,q)}  DY[(n,p,q)][k_out] * X[n, p*st-pad+r, q*st-pad+s, c]
// fwd/dgrad ("NT"): both operands K-contiguous in LDS, fragments by ds_read_b128 (XOR-swizzled rows).
// wgrad ("TN"): both operands pixel-major in LDS, fragments by ds_read_b64_tr_b16 (hardware transpose).
// MFMA: v_mfma_f32_32x32x16_bf16, 4 waves (2x2) per 256-thread block, register-staged double buffer.
#include "avt_common.h"
#include "avt_tuning.h"  // the knobs and avt_conv_fwd_plan defined here

#include <mutex>
#include <vector>

namespace avt {

#include "conv_params.h"

template <int MODE, int CVEC, int BM, int BN>
__global__ __launch_bounds__(256) void gemm_nt_kernel(GemmNTParams p) {
  constexpr int TM = BM / 64, TN = BN / 64;  // 32x32 tiles per wave (waves 2x2)
  constexpr int AR = BM / 64, BR = BN / 64;  // staged rows per thread
  constexpr int STAGE_BYTES = 2 * (BM + BN) * 64;
  constexpr int CT_LD = BN + 8;  // epilogue tile row (bf16 elements)
  constexpr int EPI_BYTES = BM * CT_LD * 2;
  constexpr int SMEM = (STAGE_BYTES > EPI_BYTES ? STAGE_BYTES : EPI_BYTES);
  __shared__ __attribute__((aligned(16))) char smem[SMEM + 4 * BN * 4];
  float* red = reinterpret_cast<float*>(smem + SMEM);  // [2][2][BN] stats scratch

  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int wm = wid >> 1, wn = wid & 1;
  const int nnt = p.Ng / BN;
  const int mt = blockIdx.x / nnt, nt = blockIdx.x % nnt;
  const int m0 = mt * BM, n0 = nt * BN;

  // ---- per-thread load assignment: chunk (tid&3) of rows (tid>>2) + 64*i ----
  const int lchunk = tid & 3, lrow = tid >> 2;
  int a_pix[AR], a_y[AR], a_x[AR];
  bool a_ok[AR];
#pragma unroll
  for (int i = 0; i < AR; ++i) {
    const int m = m0 + lrow + 64 * i;
    a_ok[i] = m < p.M;
    const int mm = a_ok[i] ? m : 0;
    const int hw = p.OH * p.OW;
    const int n = mm / hw, rem = mm - n * hw;
    const int oh = rem / p.OW, ow = rem - oh * p.OW;
    a_pix[i] = n * p.IH * p.IW;
    if (MODE == MODE_FWD) {
      a_y[i] = oh * p.stride - p.pad;
      a_x[i] = ow * p.stride - p.pad;
    } else {
      a_y[i] = oh + p.pad;
      a_x[i] = ow + p.pad;
    }
  }
  const bf16_t* bptr[BR];
#pragma unroll
  for (int i = 0; i < BR; ++i) bptr[i] = p.wmat + (size_t)(n0 + lrow + 64 * i) * p.Kg + lchunk * 8;

  u32x4 ra[AR], rb[BR];
  const int nkt = p.Kg / 32;

  auto load_tile = [&](int kt) {
    const int k0 = kt * 32;
#pragma unroll
    for (int i = 0; i < BR; ++i) rb[i] = *reinterpret_cast<const u32x4*>(bptr[i] + k0);
    if (CVEC == 8) {
      const int rs = k0 / p.IC, c0 = k0 - rs * p.IC;
      const int r = rs / p.S, s = rs - r * p.S;
#pragma unroll
      for (int i = 0; i < AR; ++i) {
        int y, x;
        bool ok = a_ok[i];
        if (MODE == MODE_FWD) {
          y = a_y[i] + r;
          x = a_x[i] + s;
        } else {
          int yn = a_y[i] - r, xn = a_x[i] - s;
          if (p.stride == 2) {
            ok = ok && ((yn & 1) == 0) && ((xn & 1) == 0);
            yn >>= 1;
            xn >>= 1;
          }
          y = yn;
          x = xn;
        }
        ok = ok && y >= 0 && y < p.IH && x >= 0 && x < p.IW;
        u32x4 v = {0u, 0u, 0u, 0u};
        if (ok) v = *reinterpret_cast<const u32x4*>(p.act + (size_t)(a_pix[i] + y * p.IW + x) * p.IC + c0 + lchunk * 8);
        ra[i] = v;
      }
    } else {
      // stems: C == CVEC (1 or 4), k = (r*S + s)*C + c; positions beyond R*S are zero padding
      const int kc = k0 + lchunk * 8;
#pragma unroll
      for (int i = 0; i < AR; ++i) {
        unsigned short e[8];
#pragma unroll
        for (int g = 0; g < 8 / CVEC; ++g) {
          const int pos = (kc + g * CVEC) / CVEC;
          const int r = pos / p.S, s = pos - r * p.S;
          const int y = a_y[i] + r, x = a_x[i] + s;
          const bool ok = a_ok[i] && pos < p.R * p.S && y >= 0 && y < p.IH && x >= 0 && x < p.IW;
          const bf16_t* src = p.act + (size_t)(a_pix[i] + y * p.IW + x) * CVEC;
          if (CVEC == 4) {
            u32x2 v = {0u, 0u};
            if (ok) v = *reinterpret_cast<const u32x2*>(src);
            e[g * 4 + 0] = v.x & 0xffff;
            e[g * 4 + 1] = v.x >> 16;
            e[g * 4 + 2] = v.y & 0xffff;
            e[g * 4 + 3] = v.y >> 16;
          } else {
            e[g] = ok ? src[0] : (unsigned short)0;
          }
        }
        u32x4 v;
        v.x = e[0] | ((unsigned)e[1] << 16);
        v.y = e[2] | ((unsigned)e[3] << 16);
        v.z = e[4] | ((unsigned)e[5] << 16);
        v.w = e[6] | ((unsigned)e[7] << 16);
        ra[i] = v;
      }
    }
  };
  auto store_tile = [&](int buf) {
    char* As = smem + buf * (BM + BN) * 64;
    char* Bs = As + BM * 64;
#pragma unroll
    for (int i = 0; i < AR; ++i) *reinterpret_cast<u32x4*>(As + swz64(lrow + 64 * i, lchunk)) = ra[i];
#pragma unroll
    for (int i = 0; i < BR; ++i) *reinterpret_cast<u32x4*>(Bs + swz64(lrow + 64 * i, lchunk)) = rb[i];
  };

  f32x16 acc[TM][TN];
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j)
#pragma unroll
      for (int v = 0; v < 16; ++v) acc[i][j][v] = 0.f;

  load_tile(0);
  store_tile(0);
  __syncthreads();
  const int frow = lane & 31, fhalf = lane >> 5;
  for (int kt = 0; kt < nkt; ++kt) {
    const int cur = kt & 1;
    if (kt + 1 < nkt) load_tile(kt + 1);
    const char* As = smem + cur * (BM + BN) * 64;
    const char* Bs = As + BM * 64;
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      bf16x8 af[TM], bfr[TN];
#pragma unroll
      for (int i = 0; i < TM; ++i) {
        const int row = wm * (BM / 2) + i * 32 + frow;
        af[i] = *reinterpret_cast<const bf16x8*>(As + swz64(row, ks * 2 + fhalf));
      }
#pragma unroll
      for (int j = 0; j < TN; ++j) {
        const int row = wn * (BN / 2) + j * 32 + frow;
        bfr[j] = *reinterpret_cast<const bf16x8*>(Bs + swz64(row, ks * 2 + fhalf));
      }
#pragma unroll
      for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af[i], bfr[j], acc[i][j], 0, 0, 0);
    }
    if (kt + 1 < nkt) store_tile(cur ^ 1);
    __syncthreads();
  }

  // ---- epilogue: BN partial statistics over valid rows (fp32, before rounding) ----
  const int rows_valid = min(BM, p.M - m0);
  if (MODE == MODE_FWD && p.stats != nullptr) {
    float colsum[TN];
#pragma unroll
    for (int j = 0; j < TN; ++j) {
      float s = 0.f;
#pragma unroll
      for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int v = 0; v < 16; ++v) {
          const int r = wm * (BM / 2) + i * 32 + (v & 3) + 8 * (v >> 2) + 4 * fhalf;
          if (r < rows_valid) s += acc[i][j][v];
        }
      s += __shfl_xor(s, 32, 64);
      colsum[j] = s;
      if (lane < 32) red[wm * BN + wn * (BN / 2) + j * 32 + lane] = s;
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < TN; ++j) {
      const int c = wn * (BN / 2) + j * 32 + frow;
      const float mean = (red[c] + red[BN + c]) / (float)rows_valid;
      float q = 0.f;
#pragma unroll
      for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int v = 0; v < 16; ++v) {
          const int r = wm * (BM / 2) + i * 32 + (v & 3) + 8 * (v >> 2) + 4 * fhalf;
          const float d = acc[i][j][v] - mean;
          if (r < rows_valid) q += d * d;
        }
      q += __shfl_xor(q, 32, 64);
      if (lane < 32) red[2 * BN + wm * BN + c] = q;
      (void)colsum;
    }
    __syncthreads();
    bn_write_header(p.stats, (p.M + BM - 1) / BM, 0, mt == 0 && n0 == 0);
    double* acc_slot = bn_fwd_slots(p.stats) + (size_t)mt * p.Ng * 3;  // this row tile's own slot
    for (int c = tid; c < BN; c += 256) {
      const double s = (double)red[c] + (double)red[BN + c];
      const double m2 = (double)red[2 * BN + c] + (double)red[3 * BN + c];
      double* a = acc_slot + (size_t)(n0 + c) * 3;
      a[0] = s;
      a[1] = m2;
      a[2] = s * s / (double)rows_valid;
    }
  }

  // ---- epilogue: bf16 tile through LDS, 16-byte coalesced stores ----
  bf16_t* Ct = reinterpret_cast<bf16_t*>(smem);
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j)
#pragma unroll
      for (int v = 0; v < 16; ++v) {
        const int r = wm * (BM / 2) + i * 32 + (v & 3) + 8 * (v >> 2) + 4 * fhalf;
        const int c = wn * (BN / 2) + j * 32 + frow;
        Ct[r * CT_LD + c] = f2bf(acc[i][j][v]);
      }
  __syncthreads();
  constexpr int CPR = BN / 8;  // 16-byte chunks per row
  for (int idx = tid; idx < BM * CPR; idx += 256) {
    const int r = idx / CPR, cc = idx - r * CPR;
    if (r >= rows_valid) continue;
    u32x4 v = *reinterpret_cast<const u32x4*>(Ct + r * CT_LD + cc * 8);
    const size_t off = (size_t)(m0 + r) * p.Ng + n0 + cc * 8;
    if (p.add != nullptr) {
      u32x4 a = *reinterpret_cast<const u32x4*>(p.add + off);
      unsigned* vv = reinterpret_cast<unsigned*>(&v);
      unsigned* aa = reinterpret_cast<unsigned*>(&a);
      if (p.amask != nullptr) {
        const unsigned bits = p.amask[off >> 3];
#pragma unroll
        for (int e = 0; e < 4; ++e)
          aa[e] &= ((bits >> (2 * e)) & 1u ? 0x0000ffffu : 0u) | ((bits >> (2 * e + 1)) & 1u ? 0xffff0000u : 0u);
      }
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const float lo = bf2f(vv[e] & 0xffff) + bf2f(aa[e] & 0xffff);
        const float hi = bf2f(vv[e] >> 16) + bf2f(aa[e] >> 16);
        vv[e] = pack2(lo, hi);
      }
    }
    *reinterpret_cast<u32x4*>(p.out + off) = v;
  }
}

// ------------------------------------------------------------------------------------------------
// TN kernel (wgrad): DW[k_out][col] += sum_pix DY[pix][k_out] * X(pix, col)
// ------------------------------------------------------------------------------------------------

template <int CVEC, int BM, int BN>
__global__ __launch_bounds__(256) void gemm_tn_kernel(GemmTNParams p) {
  constexpr int TM = BM / 64, TN = BN / 64;
  constexpr int ALD = BM + 32, BLD = BN + 32;  // row strides (elements): +64 B keeps tr reads conflict-free
  constexpr int ACPR = BM / 8, BCPR = BN / 8;  // 16-B chunks per pixel row
  constexpr int AROWS = 32 * ACPR / 256, BROWS = 32 * BCPR / 256;  // rows staged per thread
  constexpr int ASTEP = 256 / ACPR, BSTEP = 256 / BCPR;
  constexpr int BUF = 32 * (ALD + BLD);  // elements per buffer
  __shared__ __attribute__((aligned(16))) bf16_t smem[2 * BUF];

  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int wm = wid >> 1, wn = wid & 1;
  const int nnt = p.Ng / BN;
  const int mt = blockIdx.x / nnt, nt = blockIdx.x % nnt;
  const int m0 = mt * BM, n0 = nt * BN;
  const int nkt_total = (p.Kred + 31) / 32;
  const int kt_begin = blockIdx.y * p.kt_per_split;
  const int kt_end = min(nkt_total, kt_begin + p.kt_per_split);
  if (kt_begin >= kt_end) return;

  const int a_chunk = tid % ACPR, a_row = tid / ACPR;
  const int b_chunk = tid % BCPR, b_row = tid / BCPR;
  // this thread's patch columns: col = n0 + 8*b_chunk + e
  const int colbase = n0 + 8 * b_chunk;
  int b_r = 0, b_s = 0, b_c = 0;
  if (CVEC == 8) {
    const int rs = colbase / p.Cp;
    b_c = colbase - rs * p.Cp;
    b_r = rs / p.S;
    b_s = rs - b_r * p.S;
  }
  const bool b_colok = colbase < p.R * p.S * p.Cp;
  const int PQ = p.P * p.Q;

  u32x4 ra[AROWS], rb[BROWS];
  auto load_tile = [&](int kt) {
    const int pix0 = kt * 32;
#pragma unroll
    for (int i = 0; i < AROWS; ++i) {
      const int pix = pix0 + a_row + ASTEP * i;
      u32x4 v = {0u, 0u, 0u, 0u};
      if (pix < p.Kred) v = *reinterpret_cast<const u32x4*>(p.dy + (size_t)pix * p.Mg + m0 + a_chunk * 8);
      ra[i] = v;
    }
#pragma unroll
    for (int i = 0; i < BROWS; ++i) {
      const int pix = pix0 + b_row + BSTEP * i;
      const bool pok = pix < p.Kred;
      const int pp = pok ? pix : 0;
      const int n = pp / PQ, rem = pp - n * PQ;
      const int oh = rem / p.Q, ow = rem - oh * p.Q;
      const int y0 = oh * p.stride - p.pad, x0 = ow * p.stride - p.pad;
      const bf16_t* img = p.x + (size_t)n * p.H * p.W * p.Cp;
      if (CVEC == 8) {
        const int y = y0 + b_r, x = x0 + b_s;
        u32x4 v = {0u, 0u, 0u, 0u};
        if (pok && b_colok && y >= 0 && y < p.H && x >= 0 && x < p.W)
          v = *reinterpret_cast<const u32x4*>(img + (size_t)(y * p.W + x) * p.Cp + b_c);
        rb[i] = v;
      } else {
        unsigned short e[8];
#pragma unroll
        for (int g = 0; g < 8 / CVEC; ++g) {
          const int pos = (colbase + g * CVEC) / CVEC;
          const int r = pos / p.S, s = pos - r * p.S;
          const int y = y0 + r, x = x0 + s;
          const bool ok = pok && pos < p.R * p.S && y >= 0 && y < p.H && x >= 0 && x < p.W;
          const bf16_t* src = img + (size_t)(y * p.W + x) * CVEC;
          if (CVEC == 4) {
            u32x2 v = {0u, 0u};
            if (ok) v = *reinterpret_cast<const u32x2*>(src);
            e[g * 4 + 0] = v.x & 0xffff;
            e[g * 4 + 1] = v.x >> 16;
            e[g * 4 + 2] = v.y & 0xffff;
            e[g * 4 + 3] = v.y >> 16;
          } else {
            e[g] = ok ? src[0] : (unsigned short)0;
          }
        }
        u32x4 v;
        v.x = e[0] | ((unsigned)e[1] << 16);
        v.y = e[2] | ((unsigned)e[3] << 16);
        v.z = e[4] | ((unsigned)e[5] << 16);
        v.w = e[6] | ((unsigned)e[7] << 16);
        rb[i] = v;
      }
    }
  };
  auto store_tile = [&](int buf) {
    bf16_t* As = smem + buf * BUF;
    bf16_t* Bs = As + 32 * ALD;
#pragma unroll
    for (int i = 0; i < AROWS; ++i) *reinterpret_cast<u32x4*>(As + (a_row + ASTEP * i) * ALD + a_chunk * 8) = ra[i];
#pragma unroll
    for (int i = 0; i < BROWS; ++i) *reinterpret_cast<u32x4*>(Bs + (b_row + BSTEP * i) * BLD + b_chunk * 8) = rb[i];
  };

  f32x16 acc[TM][TN];
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j)
#pragma unroll
      for (int v = 0; v < 16; ++v) acc[i][j][v] = 0.f;

  // tr-read lane geometry: group g = lane>>4 (16 lanes), t = lane&15 = 4q + pp
  const int g = lane >> 4, t = lane & 15, q = t >> 2, pq = t & 3;
  const int tr_row = (g >> 1) * 8 + q;        // + 16*ks + 4*rr
  const int tr_col = (g & 1) * 16 + 4 * pq;   // + tile column base

  load_tile(kt_begin);
  store_tile(0);
  __syncthreads();
  for (int kt = kt_begin; kt < kt_end; ++kt) {
    const int cur = (kt - kt_begin) & 1;
    if (kt + 1 < kt_end) load_tile(kt + 1);
    typedef __attribute__((address_space(3))) s16x4 lds_s16x4;
    const bf16_t* As = smem + cur * BUF;
    const bf16_t* Bs = As + 32 * ALD;
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      bf16x8 af[TM], bfr[TN];
#pragma unroll
      for (int i = 0; i < TM; ++i) {
        const int col = wm * (BM / 2) + i * 32 + tr_col;
        const bf16_t* a0 = As + (ks * 16 + tr_row) * ALD + col;
        s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)(a0));
        s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)(a0 + 4 * ALD));
        short tmp[8] = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
        af[i] = __builtin_bit_cast(bf16x8, tmp);
      }
#pragma unroll
      for (int j = 0; j < TN; ++j) {
        const int col = wn * (BN / 2) + j * 32 + tr_col;
        const bf16_t* b0 = Bs + (ks * 16 + tr_row) * BLD + col;
        s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)(b0));
        s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)(b0 + 4 * BLD));
        short tmp[8] = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
        bfr[j] = __builtin_bit_cast(bf16x8, tmp);
      }
#pragma unroll
      for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af[i], bfr[j], acc[i][j], 0, 0, 0);
    }
    if (kt + 1 < kt_end) store_tile(cur ^ 1);
    __syncthreads();
  }

  // ---- epilogue: fp32 atomics into DW[k_out][(r,s,c_real)] ----
  const int ldw = p.R * p.S * p.Creal;
  const int frow = lane & 31, fhalf = lane >> 5;
#pragma unroll
  for (int j = 0; j < TN; ++j) {
    const int col = n0 + wn * (BN / 2) + j * 32 + frow;
    const int rs = col / p.Cp, c = col - rs * p.Cp;
    const bool cok = rs < p.R * p.S && c < p.Creal;
    const int dcol = rs * p.Creal + c;
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
      for (int v = 0; v < 16; ++v) {
        const int row = m0 + wm * (BM / 2) + i * 32 + (v & 3) + 8 * (v >> 2) + 4 * fhalf;
        if (cok && row < p.Mg) atomicAdd(p.dw + (size_t)row * ldw + dcol, acc[i][j][v]);
      }
  }
}

#include "conv_epi.h"
#include "conv_nt_pipe.h"
#include "conv_tn_pipe.h"
#include "conv_halo.h"
#include "conv_c64.h"
#include "conv_wgrad_halo.h"
#include "conv_stem.h"
#include "conv_stem_wgrad.h"

static int g_stem_kernel = -1;  // 7x7/s2 stem forwards on conv_stem_fwd_kernel: -1 = env AVT_STEM (default 1;
                                // 0 = the generic gather kernel, ~1.7x slower: tools/stem_bench.py)
static int stem_enabled() {
  if (g_stem_kernel < 0) {
    const char* e = getenv("AVT_STEM");
    g_stem_kernel = e ? atoi(e) : 1;
  }
  return g_stem_kernel;
}

static int g_stem_wgrad = -1;  // 7x7/s2 stem wgrads on conv_stem_wgrad_kernel: -1 = env AVT_STEM_WGRAD (default 1)

static int g_nt64_config = -1;  // tile config of the pipelined NT kernel for 64-wide GEMM N (A/B knob; -1 auto)
static int g_nt128_config = -1; // ... and for GEMM N % 128 == 0 (-1: by GEMM M, see plan_nt)
static int g_wgrad_blocks = 0;     // wgrad split-K: 0 = wave model (plan_wgrad_gemm), >0 = fixed block target
static int g_wgrad_min_kt = 4;
// largest split count that goes through a slab (deterministic: split partials summed in split order); beyond it
// fp32 atomics (non-deterministic summation order; an A/B knob only: AVT_WGRAD_SLAB_MAX / avt_set_wgrad_slab_max)
static int g_wgrad_slab_max = 1 << 30;
static int g_wgrad_wave_cost = 16; // per-block fixed cost (prologue fill + epilogue) in k-tiles
static int g_wgrad_big = -1;       // allow the 8-wave 256-wide wgrad tiles (-1: env AVT_WGRAD_BIG, default 1)
static int g_wgrad_nst = -1, g_wgrad_nst_big = -1;  // TN ring depth (4-wave / 8-wave tiles); -1: env
static int g_wgrad_slots_pct = -1;  // wgrad planner's slot share: 0 auto (by batch), 1-100 fixed, -1 env AVT_WGRAD_SLOTS_PCT
static int g_small_tile_pct = -2;  // 64-row fwd/dgrad tiles for small GEMMs (use_small_tile): % of the CUs; -2: env
static int g_wgrad_halo = -1;      // 3x3/s1 wgrad on the halo kernel (conv_wgrad_halo.h): 0 off, 1 nine taps per
                                   // block, 2 one filter row per block, 3 (default) the one-row form for K = 64
                                   // (layer 1: 480-550 -> 670-715 TFLOP/s), tap-gather elsewhere; -1 = env AVT_WGRAD_HALO
static int num_cus() {
  static int n = 0;
  if (n == 0) {
    int d = 0;
    hipDeviceProp_t pr;
    n = (hipGetDevice(&d) == hipSuccess && hipGetDeviceProperties(&pr, d) == hipSuccess && pr.multiProcessorCount > 0)
            ? pr.multiProcessorCount
            : 256;
  }
  return n;
}
static int g_halo = -1;  // 3x3/s1 fwd/dgrad on the halo-reuse kernel: -1 = env AVT_HALO (default 1)
static int halo_enabled() {
  if (g_halo < 0) {
    const char* e = getenv("AVT_HALO");
    g_halo = e ? atoi(e) : 1;
  }
  return g_halo;
}
// weight-ring stages of the layer3/4 halo tiles (A/B knobs): AVT_HALO_NST for the 128 x 128 tile (default 2:
// two blocks per CU; 3 = one block: B=128 layer3/4 -12..-20 %), AVT_HALO_SMALL_NST for the 64 x 128
// small-batch tile (default 3, still two blocks per CU: B=32 layer3 +3..16 %, vision layer4 +3..20 %;
// 4 and 5 leave one block per CU and lose; tools/conv_bench.py --stages)
static int g_halo_nst = -1, g_halo_small_nst = -1;  // -1: from the environment; avt_set_halo_stages
static int halo_nst() {
  if (g_halo_nst < 0) g_halo_nst = getenv("AVT_HALO_NST") ? atoi(getenv("AVT_HALO_NST")) : 2;
  return g_halo_nst;
}
static int halo_small_nst() {
  if (g_halo_small_nst < 0) g_halo_small_nst = getenv("AVT_HALO_SMALL_NST") ? atoi(getenv("AVT_HALO_SMALL_NST")) : 3;
  return g_halo_small_nst;
}
// the 8-wave 256 x 128 halo tile (one block per CU) in place of the 128 x 128 one where measured faster
// (tools/conv_bench.py --halo 1,2; B=128): layer4 (K = 4608: V +5..7 %, A +6..7 %; B=32 A +9 %) and GEMMs
// whose 256-row tiles fit one wave of blocks (vision layer3: +7..11 %); the audio layer3 GEMM
// (324 tiles, 1.3 waves) loses 13 %.  AVT_HALO8=0 keeps the 128 x 128 tile everywhere.
static int g_halo8 = -1;
static bool halo8_pick(const GemmNTParams& p) {
  if (g_halo8 < 0) g_halo8 = getenv("AVT_HALO8") ? atoi(getenv("AVT_HALO8")) : 1;
  if (!g_halo8) return false;
  if (p.IC >= 512) return true;
  // (A/B, env AVT_HALO8_PCT, default 100: the grid of 256-row tiles may reach that % of the CUs -- in the step the
  // other trunk's kernels fill a partial second round)
  static const int pct = getenv("AVT_HALO8_PCT") ? atoi(getenv("AVT_HALO8_PCT")) : 100;
  return (long)((p.M + 255) / 256) * (p.Ng / 128) * 100 <= (long)num_cus() * pct;
}
// weight-ring stages of the 8-wave 256 x 128 halo tile (A/B knob AVT_HALO8_NST: 3 default, or 4 -- the tile runs
// one block per CU either way, so a fourth stage is one more weight tile in flight for free LDS)
static int g_halo8_nst = -1;  // -1: env AVT_HALO8_NST (default 3)
static int halo8_nst() {
  if (g_halo8_nst < 0) g_halo8_nst = getenv("AVT_HALO8_NST") ? atoi(getenv("AVT_HALO8_NST")) : 3;
  return g_halo8_nst;
}
// wave layout of the 256 x 128 halo tile (A/B knob AVT_HALO8_FORM): 0 = 8 waves of 64 x 64 (TM = TN = 2: every
// fragment read feeds two MFMAs, 1 KB of LDS reads per MFMA), 1 = 4 waves of 128 x 64 (TM = 4, TN = 2: 0.75 KB per
// MFMA, one wave per SIMD with the whole register file)
static int g_halo8_form = -1;  // -1: env AVT_HALO8_FORM (default 0)
static int halo8_form() {
  if (g_halo8_form < 0) g_halo8_form = getenv("AVT_HALO8_FORM") ? atoi(getenv("AVT_HALO8_FORM")) : 0;
  return g_halo8_form;
}
static int g_c64 = -1;  // layer-1 (C = K = 64, 3x3/s1) fwd/dgrad on conv_c64_kernel: -1 = env AVT_C64 (default 1)
static int c64_enabled() {
  if (g_c64 < 0) {
    const char* e = getenv("AVT_C64");
    g_c64 = e ? atoi(e) : 1;
  }
  return g_c64;
}

static int g_s2_one = -1;  // stride-2 dgrad parity classes in one launch: -1 = env AVT_S2_ONE (default 1)
static int s2_one() {
  if (g_s2_one < 0) {
    const char* e = getenv("AVT_S2_ONE");
    g_s2_one = e ? atoi(e) : 1;
  }
  return g_s2_one;
}

static int g_conv_variant = -1;  // -1: read AVT_CONV_VARIANT once (0 = register-staged, 1 = LDS-DMA)
static int conv_variant() {
  if (g_conv_variant < 0) {
    const char* e = getenv("AVT_CONV_VARIANT");
    g_conv_variant = e ? atoi(e) : 1;
  }
  return g_conv_variant;
}

}  // namespace avt

using namespace avt;

extern "C" int avt_set_conv_variant(int v) {
  avt::g_conv_variant = v;
  return AVT_OK;
}

extern "C" int avt_set_c64(int on) {
  g_c64 = on ? 1 : 0;
  return AVT_OK;
}

extern "C" int avt_set_s2_dgrad_one(int on) {
  g_s2_one = on ? 1 : 0;
  return AVT_OK;
}

extern "C" int avt_set_halo(int on) {
  avt::g_halo = on < 0 ? 0 : (on > 2 ? 2 : on);
  return AVT_OK;
}

extern "C" int avt_set_halo8(int on) {
  avt::g_halo8 = on < 0 ? -1 : (on ? 1 : 0);
  return AVT_OK;
}

extern "C" int avt_set_halo_stages(int nst128, int nst64) {
  AVT_REQUIRE(nst128 >= 2 && nst128 <= 5 && nst64 >= 2 && nst64 <= 5, "set_halo_stages: nst128, nst64 in 2..5");
  avt::g_halo_nst = nst128;
  avt::g_halo_small_nst = nst64;
  return AVT_OK;
}

extern "C" int avt_set_nt64_config(int cfg) {
  AVT_REQUIRE(cfg >= -1 && cfg <= 8, "set_nt64_config: cfg in -1..8");
  g_nt64_config = cfg;
  return AVT_OK;
}

extern "C" int avt_set_nt128_config(int cfg) {
  AVT_REQUIRE(cfg >= -1 && cfg <= 6, "set_nt128_config: cfg=%d out of range", cfg);
  avt::g_nt128_config = cfg;
  return AVT_OK;
}

extern "C" int avt_set_wgrad_policy(int target_blocks, int min_ktiles) {
  AVT_REQUIRE(target_blocks >= 0 && min_ktiles >= 1, "set_wgrad_policy: bad arguments");
  avt::g_wgrad_blocks = target_blocks;
  avt::g_wgrad_min_kt = min_ktiles;
  return AVT_OK;
}

extern "C" int avt_set_wgrad_slab_max(int max_splits, int wave_cost) {
  AVT_REQUIRE(max_splits >= 0 && wave_cost >= 0, "set_wgrad_slab_max: bad arguments");
  avt::g_wgrad_slab_max = max_splits;
  avt::g_wgrad_wave_cost = wave_cost;
  return AVT_OK;
}

extern "C" int avt_set_stem_wgrad(int on) {
  avt::g_stem_wgrad = on ? 1 : 0;
  return AVT_OK;
}

extern "C" int avt_set_stem_kernel(int on) {
  avt::g_stem_kernel = on ? 1 : 0;
  return AVT_OK;
}

extern "C" int avt_set_small_tiles(int waves) {
  AVT_REQUIRE(waves >= -2 && waves <= 64, "avt_set_small_tiles: %d (blocks per CU; 0 never, -1 always, -2 env)", waves);
  avt::g_small_tile_pct = waves > 0 ? 100 * waves : waves;
  return AVT_OK;
}

extern "C" int avt_set_wgrad_tiles(int big) {
  avt::g_wgrad_big = big ? 1 : 0;
  return AVT_OK;
}

// TN wgrad ring depth: nst for the 4-wave tiles (4, 6 or 8), nst_big for the 8-wave 256 x 256 tile (3-5)
extern "C" int avt_set_wgrad_nst(int nst, int nst_big) {
  AVT_REQUIRE(nst >= 4 && nst <= 8 && nst_big >= 3 && nst_big <= 5, "set_wgrad_nst: nst in 4..8, nst_big in 3..5");
  avt::g_wgrad_nst = nst;
  avt::g_wgrad_nst_big = nst_big;
  return AVT_OK;
}

// share of the chip's block slots the tap-gather wgrad's split planner assumes: 0 auto (65 % at batch <= 32, 75 % at
// <= 64, else 100 %), 1-100 fixed, -1 back to env AVT_WGRAD_SLOTS_PCT.  Size workspaces after changing it.
extern "C" int avt_set_wgrad_slots_pct(int pct) {
  AVT_REQUIRE(pct >= -1 && pct <= 100, "avt_set_wgrad_slots_pct: %d (0 auto, 1-100 fixed, -1 env)", pct);
  avt::g_wgrad_slots_pct = pct;
  return AVT_OK;
}

// ------------------------------------------------------------------------------------------------
// C-ABI
// ------------------------------------------------------------------------------------------------
static inline int conv_out(int in, int k, int st, int pad) { return (in + 2 * pad - k) / st + 1; }

// the store epilogue of a fwd/dgrad launch (the values of avt_conv_fwd_plan's `epi`, include/avt_tuning.h): plain
// (BN statistics, add, BN-backward), the bias epilogue on the 2-D kernels' narrow argument form (at most 9 taps),
// the bias epilogue on the Conv3d / long-tap-list form
enum { EPI_PLAIN = 0, EPI_BIAS2D = 1, EPI_BIAS3D = 2 };

// BIAS: the bias-epilogue instantiations; VIDB picks their Conv3d / long-tap-list form (avt_conv3d_fwd_bias)
template <int MODE, int WM, int WN, int TM, int TN, int NST, int BK, bool BIAS = false, bool VIDB = false>
static bool launch_pipe_one(const GemmNTParams& p, const NTPipeArgsV& ta0, hipStream_t st) {
  constexpr int BM = WM * TM * 32, BN = WN * TN * 32;
  const int grid = ((p.M + BM - 1) / BM) * (p.Ng / BN);
  if (grid <= 0) return true;
  NTPipeArgsV ta = ta0;  // the output grid's row divisors (per parity class for a multi-class dgrad)
  ta.div_hw = make_magic((unsigned)(p.OH * p.OW));
  ta.div_ow = make_magic((unsigned)p.OW);
  for (int k = 0; k < 4; ++k) {
    const int ph = (ta.cls_meta[k] >> 8) & 1, pw = (ta.cls_meta[k] >> 9) & 1;
    const int oh = (ta.OHf - ph + 1) >> 1, ow = (ta.OWf - pw + 1) >> 1;
    ta.cdiv_hw[k] = make_magic((unsigned)(oh > 0 && ow > 0 ? oh * ow : 1));
    ta.cdiv_ow[k] = make_magic((unsigned)(ow > 0 ? ow : 1));
  }
  if constexpr (BIAS && VIDB) {  // avt_conv3d_fwd_bias: Conv3d rows, up to kMaxTaps taps
    hipLaunchKernelGGL((conv_nt_pipe_kernel<MODE, WM, WN, TM, TN, NST, BK, true, false, true>), dim3(grid),
                       dim3(WM * WN * 64), 0, st, p, ta);
  } else if constexpr (BIAS) {  // avt_conv2d_fwd_bias: a 2-D forward of at most 9 taps
    hipLaunchKernelGGL((conv_nt_pipe_kernel<MODE, WM, WN, TM, TN, NST, BK, false, false, true>), dim3(grid),
                       dim3(WM * WN * 64), 0, st, p, narrow_args(ta));
  } else if (p.IT > 1 || p.OT > 1 || p.KT > 1 || ta.ntaps > 9) {
    // Conv3d, and every 2-D conv of more than 9 taps (5x5, 1x7, the folded 49-tap video stem): the 2-D instantiations
    // take the 9-tap argument block, and narrow_args() keeps nine taps.  Forward only: the dgrad entry points refuse
    // a launch of more than 9 taps.
    if constexpr (MODE == MODE_FWD)
      hipLaunchKernelGGL((conv_nt_pipe_kernel<MODE, WM, WN, TM, TN, NST, BK, true>), dim3(grid), dim3(WM * WN * 64), 0,
                         st, p, ta);
    else
      return false;  // no long-tap-list dgrad instantiation: the caller reports "no kernel for the plan"
  } else if (MODE == MODE_DGRAD && p.bx != nullptr) {
    hipLaunchKernelGGL((conv_nt_pipe_kernel<MODE, WM, WN, TM, TN, NST, BK, false, true>), dim3(grid),
                       dim3(WM * WN * 64), 0, st, p, narrow_args(ta));
  } else {
    hipLaunchKernelGGL((conv_nt_pipe_kernel<MODE, WM, WN, TM, TN, NST, BK>), dim3(grid), dim3(WM * WN * 64), 0, st, p,
                       narrow_args(ta));
  }
  return true;
}

// The tap list of a forward or a stride-1 dgrad: all KT*R*S taps in weight order, each displaced by
// (kt, r, s) - pad (forward) or pad - (kt, r, s) (dgrad).  A 2-D conv is KT = 1, pad_t = 0.
static void fill_taps(NTPipeArgsV& ta, const GemmNTParams& p, int mode) {
  const int sgn = mode == MODE_FWD ? 1 : -1;
  ta.ntaps = p.KT * p.R * p.S;
  for (int kt = 0; kt < p.KT; ++kt)
    for (int r = 0; r < p.R; ++r)
      for (int s = 0; s < p.S; ++s) {
        const int t = (kt * p.R + r) * p.S + s;
        ta.tap_w[t] = t;
        ta.tap_dt[t] = sgn * (kt - p.pad_t);
        ta.tap_dy[t] = sgn * (r - p.pad);
        ta.tap_dx[t] = sgn * (s - p.pad);
      }
}

// Builds the tap list(s) and launches: fwd / stride-1 dgrad in one launch (EPI: on the plain or a bias-epilogue
// instantiation); a stride-2 dgrad as four parity-class launches, each walking only its class's taps.
// BK = 64 needs whole 64-channel taps (IC % 64 == 0: plan_nt sees to it).  False: a launch had no instantiation.
template <int MODE, int WM, int WN, int TM, int TN, int NST, int BK, int EPI = EPI_PLAIN>
static bool launch_glds(const GemmNTParams& p, hipStream_t st) {
  NTPipeArgsV ta{};
  const int batch = p.M / (p.OT * p.OH * p.OW);
  ta.act_bytes = (unsigned)((size_t)batch * p.IT * p.IH * p.IW * p.IC * 2);
  ta.w_bytes = (unsigned)((size_t)p.Ng * p.Kg * 2);
  if (MODE == MODE_FWD || p.stride == 1) {
    fill_taps(ta, p, MODE);
    return launch_pipe_one<MODE, WM, WN, TM, TN, NST, BK, EPI != EPI_PLAIN, EPI == EPI_BIAS3D>(p, ta, st);
  }
  ta.cls = 1;
  ta.OHf = p.OH;
  ta.OWf = p.OW;
  // one launch for all classes (no BN-backward epilogue): blocks of the classes with the most taps
  // are dispatched first, and the classes' tails overlap instead of running as four short grids
  if (s2_one() && p.bx == nullptr && p.R * p.S <= 9) {
    struct Cls { int ph, pw, n, tiles; } cl[4];
    int ncl = 0;
    constexpr int BM = WM * TM * 32, BN = WN * TN * 32;
    for (int ph = 0; ph < 2; ++ph)
      for (int pw = 0; pw < 2; ++pw) {
        int n = 0;
        for (int r = 0; r < p.R; ++r)
          for (int s = 0; s < p.S; ++s) n += !(((ph + p.pad - r) & 1) || ((pw + p.pad - s) & 1));
        const int m = batch * ((p.OH - ph + 1) / 2) * ((p.OW - pw + 1) / 2);
        if (m == 0 || (n == 0 && p.add != nullptr && p.add == p.out)) continue;  // see below
        cl[ncl++] = Cls{ph, pw, n, ((m + BM - 1) / BM) * (p.Ng / BN)};
      }
    for (int i = 1; i < ncl; ++i)  // most taps first (stable)
      for (int j = i; j > 0 && cl[j].n > cl[j - 1].n; --j) std::swap(cl[j], cl[j - 1]);
    NTPipeArgsV tc = ta;
    tc.ncls = ncl;
    tc.batch = batch;
    tc.ntaps = 0;
    int start = 0;
    for (int k = 0; k < ncl; ++k) {
      const int first = tc.ntaps;
      for (int r = 0; r < p.R; ++r)
        for (int s = 0; s < p.S; ++s) {
          if (((cl[k].ph + p.pad - r) & 1) || ((cl[k].pw + p.pad - s) & 1)) continue;
          tc.tap_w[tc.ntaps] = r * p.S + s;
          tc.tap_dy[tc.ntaps] = (cl[k].ph + p.pad - r) / 2;
          tc.tap_dx[tc.ntaps] = (cl[k].pw + p.pad - s) / 2;
          ++tc.ntaps;
        }
      tc.cls_start[k] = start;
      tc.cls_meta[k] = cl[k].n | first << 4 | cl[k].ph << 8 | cl[k].pw << 9;
      start += cl[k].tiles;
    }
    if (ncl == 0 || start == 0) return true;
    tc.ph = cl[0].ph;  // ncls == 1: the plain class mode (then tc.ntaps == cl[0].n)
    tc.pw = cl[0].pw;
    GemmNTParams pc = p;
    pc.OH = (p.OH - cl[0].ph + 1) / 2;
    pc.OW = (p.OW - cl[0].pw + 1) / 2;
    pc.M = batch * pc.OH * pc.OW;
    if (ncl > 1) pc.M = start / (p.Ng / BN) * BM;  // launch_pipe_one's grid = start; each block takes its class's M
    return launch_pipe_one<MODE, WM, WN, TM, TN, NST, BK>(pc, tc, st);
  }
  // the class launches that carry the BN-backward epilogue store their partial sums into consecutive
  // slot ranges of one accumulator (conv_epi.h): pass 0 counts the call's slots, pass 1 launches
  constexpr int BMc = WM * TM * 32, BNc = WN * TN * 32;
  int ep_total = 0, ep_base = 0;
  bool ok = true;
  for (int pass = 0; pass < 2; ++pass)
    for (int ph = 0; ph < 2; ++ph)
      for (int pw = 0; pw < 2; ++pw) {
        NTPipeArgsV tc = ta;
        tc.ph = ph;
        tc.pw = pw;
        tc.ntaps = 0;
        for (int r = 0; r < p.R; ++r)
          for (int s = 0; s < p.S; ++s) {
            if (((ph + p.pad - r) & 1) || ((pw + p.pad - s) & 1)) continue;
            tc.tap_w[tc.ntaps] = r * p.S + s;
            tc.tap_dy[tc.ntaps] = (ph + p.pad - r) / 2;
            tc.tap_dx[tc.ntaps] = (pw + p.pad - s) / 2;
            ++tc.ntaps;
          }
        GemmNTParams pc = p;
        if (p.bskip00 && ph == 0 && pw == 0) pc.bx = pc.bx2 = nullptr;
        pc.OH = (p.OH - ph + 1) / 2;
        pc.OW = (p.OW - pw + 1) / 2;
        pc.M = batch * pc.OH * pc.OW;
        // a class no tap reaches (e.g. 3 of the 4 classes of a 1x1/s2 downsample) runs with an empty
        // K loop: its rows are written as 0 (+ add) -- or, accumulating in place (add == out), are
        // already final and are skipped
        if (tc.ntaps == 0 && p.add != nullptr && p.add == p.out) continue;
        const int rtiles = (pc.M + BMc - 1) / BMc;  // the class's row tiles = its statistic slots
        if (rtiles * (p.Ng / BNc) <= 0) continue;
        if (pass == 0) {
          if (pc.bx != nullptr) ep_total += rtiles;
          continue;
        }
        pc.bslot_base = ep_base;
        pc.bslot_total = ep_total;
        if (pc.bx != nullptr) ep_base += rtiles;
        ok = launch_pipe_one<MODE, WM, WN, TM, TN, NST, BK>(pc, tc, st) && ok;
      }
  return ok;
}

constexpr int kHaloPR = 416;  // patch rows the halo kernels' LDS holds: 256 + 2W + 2 <= 416 -> W <= 79
// the patch of a 128-row tile fits 168 rows (W <= 19: the 4-wave 128 x 128 tile at two blocks per CU), that of a
// 256-row tile 336 (W <= 39: room for a third weight stage)
static bool halo128_fits(const GemmNTParams& p) { return 128 + 2 * p.OW + 2 <= 168; }
static bool halo256_short(const GemmNTParams& p) { return 256 + 2 * p.OW + 2 <= 336; }

// 3x3 / stride 1 / pad 1 Conv2d, 64-channel multiples, image width <= 79: the halo-reuse kernel
static bool halo_eligible(const GemmNTParams& p) {
  const int h = halo_enabled();
  if (!h || p.R != 3 || p.S != 3 || p.stride != 1 || p.pad != 1 || p.IC % 64 != 0 || p.IT > 1 || p.OT > 1 || p.KT > 1 ||
      p.IH != p.OH || p.IW != p.OW)
    return false;
  if (h == 2) return 256 + 2 * p.OW + 2 <= kHaloPR && (p.Ng % 128 == 0 || p.Ng == 64);  // 8-wave forms (A/B)
  // W <= 19 (layer3/4): 4-wave 128x128; W <= 79 (layer2): 8-wave 256x128 (measured with the unrolled tap
  // loop: audio layer2 +6-10 % at B=128 and +28 % at B=32 over the tap gather, vision layer2 +0-6 %)
  static const int l2 = getenv("AVT_HALO_L2") ? atoi(getenv("AVT_HALO_L2")) : 1;  // A/B: 0 = layer2 on the tap gather
  return p.Ng % 128 == 0 && (halo128_fits(p) || (l2 && 256 + 2 * p.OW + 2 <= kHaloPR));
}

// Small GEMMs (a few clips per GPU: BASELINE configs[2] runs 32 per GPU): a tile grid that leaves
// most of the 256 CUs idle loses more than a smaller tile's lower reuse costs.  Rows per tile drop
// from 128 to 64 when the 128-row grid would not give g_small_tile_pct % of the CUs a block.
// Measured per shape (tools/conv_bench.py --small): a 128-row grid of fewer blocks than CUs runs faster alone on
// 64-row tiles (e.g. B=32 layer3 263 -> 354 TFLOP/s), one of 1-2 blocks per CU does not (B=32 audio layer4 769 ->
// 541).  In the step the other trunk's kernels take the CUs a 128-row grid leaves: at 100 % (rounds 2-5) the
// 64-row tiles lost 1.6 % at B=32 and 0.5 % at B=64 against none, and gained 2.2 % on the tube step's 8-clip audio
// trunk (profiles/r6_ab_small_tiles*.txt); the default is AVT_SMALL_TILES_PCT (50).  avt_set_small_tiles(w) / env
// AVT_SMALL_TILES = w blocks per CU (100 w %), 0 never, -1 always.
static bool use_small_tile(const GemmNTParams& p, int BN) {
  if (g_small_tile_pct == -2) {
    const char* e = getenv("AVT_SMALL_TILES");
    const char* ep = getenv("AVT_SMALL_TILES_PCT");
    const int w = e ? atoi(e) : 1;
    g_small_tile_pct = e ? (w > 0 ? 100 * w : w) : ep ? atoi(ep) : 50;
  }
  if (g_small_tile_pct == 0) return false;
  if (g_small_tile_pct < 0) return true;
  const long long blocks128 = (long long)((p.M + 127) / 128) * (p.Ng / BN);
  return blocks128 * 100 < (long long)g_small_tile_pct * num_cus();
}

template <int MODE, int WM, int WN, int TM, int TN, int NSTB, int PRMAX, bool EPI, int OPT = 0, bool BIAS = false>
static void launch_halo_one(const GemmNTParams& p, const HaloArgs& ha, int grid, hipStream_t st) {
  hipLaunchKernelGGL((conv_halo_kernel<MODE, WM, WN, TM, TN, NSTB, PRMAX, EPI, false, 0, OPT, BIAS>), dim3(grid),
                     dim3(WM * WN * 64), 0, st, p, ha);
}

// OPT 4: the Conv3d 3x3x3 / stride 1 / pad 1 form (conv_halo.h; forward only)
// BIAS: the bias-epilogue instantiation (avt_conv2d_fwd_bias; forward, no split-K)
template <int MODE, int WM, int WN, int TM, int TN, int NSTB = 3, int PRMAX = kHaloPR, int OPT = 0, bool BIAS = false>
static void launch_halo(const GemmNTParams& p, hipStream_t st, int ksplit = 1, float* part = nullptr,
                        int* cnt = nullptr) {
  constexpr int BM = WM * TM * 32, BN = WN * TN * 32;
  HaloArgs ha{};
  ha.ksplit = ksplit;
  ha.cps = p.IC / 64 / ksplit;
#ifdef AVT_DIAG  // wrong-results timing diagnostics: the -DAVT_DIAG build only
  static const int hdbg = getenv("AVT_HALO_DBG") ? atoi(getenv("AVT_HALO_DBG")) : 0;
  ha.dbg = hdbg;
#endif
  ha.part = part;
  ha.cnt = cnt;
  const int batch = p.M / (p.OH * p.OW);
  ha.act_bytes = (unsigned)((size_t)batch * p.IH * p.IW * p.IC * 2);
  ha.w_bytes = (unsigned)((size_t)p.Ng * p.Kg * 2);
  ha.W = p.OW;
  ha.H = p.OH;
  for (int r = 0; r < 3; ++r)
    for (int s = 0; s < 3; ++s) {
      const int t = r * 3 + s;
      const int dy = MODE == MODE_FWD ? r - 1 : 1 - r, dx = MODE == MODE_FWD ? s - 1 : 1 - s;
      ha.tap_dy[t] = dy;
      ha.tap_dx[t] = dx;
      ha.tap_disp[t] = dy * p.OW + dx;
      ha.tap_w[t] = t;
    }
  if constexpr ((OPT & 4) != 0) {
    ha.T = p.IT;
    ha.div_hw = make_magic((unsigned)(p.OH * p.OW));
    ha.div_t = make_magic((unsigned)p.IT);
  }
  const int grid = ((p.M + BM - 1) / BM) * (p.Ng / BN) * ksplit;
  if constexpr (!BIAS) {
    if (grid > 0 && ksplit > 1) {
      hipLaunchKernelGGL((conv_halo_kernel<MODE, WM, WN, TM, TN, NSTB, PRMAX, false, true>), dim3(grid),
                         dim3(WM * WN * 64), 0, st, p, ha);
      return;
    }
  }
  if (grid <= 0) return;
  if constexpr (BIAS)
    launch_halo_one<MODE, WM, WN, TM, TN, NSTB, PRMAX, false, OPT, true>(p, ha, grid, st);
  else if constexpr ((OPT & 4) != 0)
    launch_halo_one<MODE, WM, WN, TM, TN, NSTB, PRMAX, false, OPT>(p, ha, grid, st);
  else if (MODE == MODE_DGRAD && p.bx != nullptr)
    launch_halo_one<MODE, WM, WN, TM, TN, NSTB, PRMAX, true, OPT>(p, ha, grid, st);
  else
    launch_halo_one<MODE, WM, WN, TM, TN, NSTB, PRMAX, false, OPT>(p, ha, grid, st);
}

// A/B knob: the 8-wave 256 x 128 halo tile with two taps per barrier and waves 4-7 at s_setprio 1 (conv_halo.h OPT 3)
// for the long-K convs (>= 8 (virtual) chunks: the 2-D layer4, C = 512; the Conv3d layer3/4).  +3..11 % per shape at
// B=128 in tools/halo_bench on random operands (profiles/r6_halo_bench_prio_tps2.txt), but +-0.1 % on the B=128 step
// (profiles/r6_ab_tps2_b128.txt) and +-2 % on the Conv3d shapes (r6_conv3d_halo.txt): off by default.
// avt_set_halo_tps2 / env AVT_HALO_TPS2 (0 default, 1 on; -1 back to the environment)
static int g_halo_tps2 = -1;
static int halo_tps2() {
  if (g_halo_tps2 < 0) g_halo_tps2 = getenv("AVT_HALO_TPS2") ? atoi(getenv("AVT_HALO_TPS2")) : 0;
  return g_halo_tps2;
}
static bool halo_tps2_shape(const GemmNTParams& p, int vt = 1) {  // vt: virtual chunks per 64 channels (Conv3d: 3)
  const int nv = p.IC / 64 * vt;
  return p.IC % 64 == 0 && nv % 2 == 0 && nv >= 8;
}

// Conv3d 3x3x3 / stride 1 / pad 1 with T' = T on the halo kernel's three-patch form: the R3D-18 layer2-4 convs (N %
// 128 == 0, W <= 79; 256 x 128 tile) and layer1 (N = 64, W <= 115; 256 x 64 tile).  Per shape at b=8 x 16 frames
// (profiles/r6_conv3d_halo.txt) 1094-1209 TFLOP/s against 886-928 for the tap gather on layer2-4, 789 against 549-635 on
// layer1.  avt_set_halo3d / env AVT_HALO3D: 2 (default) both, 1 layer2-4 only, 0 the tap-gather kernel
static int g_halo3d = -1;
static int halo3d_enabled() {
  if (g_halo3d < 0) g_halo3d = getenv("AVT_HALO3D") ? atoi(getenv("AVT_HALO3D")) : 2;
  return g_halo3d;
}
static bool halo3d_eligible(const GemmNTParams& p) {
  if (!halo3d_enabled() || p.KT != 3 || p.R != 3 || p.S != 3 || p.stride != 1 || p.pad != 1 || p.pad_t != 1 ||
      p.IT != p.OT || p.IH != p.OH || p.IW != p.OW || p.IC % 64 != 0 || conv_variant() != 1)
    return false;
  // R3D-18 layer1 (K = 64, W = 112): a 488-row patch (W <= 115)
  if (p.Ng == 64) return halo3d_enabled() >= 2 && 256 + 2 * p.OW + 2 <= 488;
  return p.Ng % 128 == 0 && 256 + 2 * p.OW + 2 <= kHaloPR;
}

// ---- split-K for the 128 x 128 halo tile (layer3/4 at a few clips per GPU) ----
// A 128-row grid of fewer blocks than the chip holds leaves CUs idle, and the 64-row tile that fills
// it moves twice the weight bytes per FLOP through L2 -> LDS.  Split-K keeps the 128 x 128 tile and
// gives each of `ksplit` blocks per tile a range of the 64-channel chunks; the last block to finish a
// tile sums the fp32 partials (conv_halo.h).  Plan: ksplit = the smallest divisor of the chunk count
// whose grid reaches g_splitk_blocks (AVT_SPLITK_BLOCKS, default 2 blocks per CU); AVT_HALO_SPLITK /
// avt_set_halo_splitk(s > 0) forces the largest divisor <= s, 1 turns it off.
static int g_halo_splitk = -1, g_splitk_blocks = -1;
struct SplitWs {
  float* part;
  int* cnt;
  long long part_floats;  // sizes the caller allocated (avt_conv2d_splitk_plan at the time of the call)
  int counters;
};
static bool halo_splitk_shape(const GemmNTParams& p) {
  return halo_eligible(p) && conv_variant() == 1 && p.Ng % 128 == 0 && halo128_fits(p) &&
         p.bx == nullptr;
}
static int halo_splitk(const GemmNTParams& p) {
  if (g_halo_splitk < 0) g_halo_splitk = getenv("AVT_HALO_SPLITK") ? atoi(getenv("AVT_HALO_SPLITK")) : 0;
  if (g_splitk_blocks < 0)
    g_splitk_blocks = getenv("AVT_SPLITK_BLOCKS") ? atoi(getenv("AVT_SPLITK_BLOCKS")) : 2 * num_cus();
  if (!halo_splitk_shape(p)) return 1;
  const int nchunk = p.IC / 64;
  const long long tiles = (long long)((p.M + 127) / 128) * (p.Ng / 128);
  if (g_halo_splitk > 0) {
    int s = 1;
    for (int d = 1; d <= nchunk && d <= g_halo_splitk; ++d)
      if (nchunk % d == 0) s = d;
    return s;
  }
  if (tiles >= g_splitk_blocks) return 1;
  int s = 1;
  for (int d = 2; d <= nchunk; ++d)
    if (nchunk % d == 0) {
      s = d;
      if (tiles * d >= g_splitk_blocks) break;
    }
  return s;
}

// C = K = 64 3x3/s1/p1 Conv2d (the layer-1 convs), image width <= 95, not a BN-epilogue dgrad and not
// in-place: the persistent resident-weight kernel (conv_c64.h); off with the halo kernels (halo 0: the
// tap-gather kernel everywhere, as the bitwise-order tests need) or avt_set_c64(0)
static bool c64_eligible(const GemmNTParams& p) {
  return c64_enabled() && halo_enabled() && conv_variant() == 1 && p.IC == 64 && p.Ng == 64 && p.Kg == 576 &&
         p.R == 3 && p.S == 3 && p.stride == 1 && p.pad == 1 && p.IT == 1 && p.OT == 1 && p.KT == 1 && p.IH == p.OH &&
         p.IW == p.OW && 256 + 2 * p.OW + 2 <= c64::PRMAX && p.bx == nullptr && (p.add == nullptr || p.add != p.out);
}

// 8-wave blocks (two waves per SIMD; default): layer-1 fwd/dgrad 519/630 -> 638/762 TFLOP/s (vision), step
// 12.61 k -> 12.86 k clips/s in the same-box A/B; AVT_C64_WAVES=4: the 4-wave form
static int c64_waves() {
  static const int w = getenv("AVT_C64_WAVES") && atoi(getenv("AVT_C64_WAVES")) == 4 ? 4 : 8;
  return w;
}

// BIAS: the bias-epilogue instantiation (avt_conv2d_fwd_bias; conv_c64_kernel's ADD 3, 8 waves only)
template <int MODE, bool BIAS = false>
static void launch_c64(const GemmNTParams& p, hipStream_t st, int waves) {
  C64Args ca{};
  const int batch = p.M / (p.OH * p.OW);
  ca.act_bytes = (unsigned)((size_t)batch * p.IH * p.IW * 64 * 2);
  ca.w_bytes = (unsigned)((size_t)64 * 576 * 2);
  ca.W = p.OW;
  ca.H = p.OH;
  ca.tiles = (p.M + c64::BM - 1) / c64::BM;
#ifdef AVT_DIAG  // wrong-results timing diagnostics: the -DAVT_DIAG build only
  static const int dbg = getenv("AVT_C64_DBG") ? atoi(getenv("AVT_C64_DBG")) : 0;
  ca.dbg = dbg;
#else
  ca.dbg = 0;
#endif
  for (int r = 0; r < 3; ++r)
    for (int s = 0; s < 3; ++s) {
      const int t = r * 3 + s;
      const int dy = MODE == MODE_FWD ? r - 1 : 1 - r, dx = MODE == MODE_FWD ? s - 1 : 1 - s;
      ca.tap_dy[t] = dy;
      ca.tap_dx[t] = dx;
    }
  // as few blocks as the same number of tile rounds needs (1568 vision tiles at B=128: 7 rounds on 224
  // blocks, not 6.1 on 256): the CUs left over take the other trunk's concurrent kernels
  // (A/B, env AVT_C64_SHARE, default 100: the share of the CUs the persistent grid may take -- the rest run the
  // other trunk's kernels)
  static const int c64_share = getenv("AVT_C64_SHARE") ? atoi(getenv("AVT_C64_SHARE")) : 100;
  const int cus = max(1, num_cus() * min(max(c64_share, 1), 100) / 100);
  const int rounds = (ca.tiles + cus - 1) / cus;
  const int grid = rounds > 0 ? (ca.tiles + rounds - 1) / rounds : 0;
  if (grid <= 0) return;
  if constexpr (BIAS) {
    hipLaunchKernelGGL((conv_c64_kernel<MODE_FWD, 3, 8>), dim3(grid), dim3(512), 0, st, p, ca);
    return;
  }
  const bool w8 = waves != 4;
  if constexpr (MODE == MODE_DGRAD) {
    if (p.add != nullptr && p.amask != nullptr) {
      if (w8)
        hipLaunchKernelGGL((conv_c64_kernel<MODE, 2, 8>), dim3(grid), dim3(512), 0, st, p, ca);
      else
        hipLaunchKernelGGL((conv_c64_kernel<MODE, 2>), dim3(grid), dim3(256), 0, st, p, ca);
      return;
    }
    if (p.add != nullptr) {
      if (w8)
        hipLaunchKernelGGL((conv_c64_kernel<MODE, 1, 8>), dim3(grid), dim3(512), 0, st, p, ca);
      else
        hipLaunchKernelGGL((conv_c64_kernel<MODE, 1>), dim3(grid), dim3(256), 0, st, p, ca);
      return;
    }
  }
  if (w8)
    hipLaunchKernelGGL((conv_c64_kernel<MODE, 0, 8>), dim3(grid), dim3(512), 0, st, p, ca);
  else
    hipLaunchKernelGGL((conv_c64_kernel<MODE, 0>), dim3(grid), dim3(256), 0, st, p, ca);
}

// ---- the fwd/dgrad plan: kernel family and tile of a call (plan_nt), and its launch (launch_plan) ----
enum { NT_C64 = 0, NT_HALO = 1, NT_HALO3D = 2, NT_GATHER = 3, NT_REG = 4, NT_STEM = 5 };  // avt_conv_fwd_plan's family
struct NtPlan {
  int family;
  int wm, wn, tm, tn;  // waves per block (rows x columns), 32 x 32 MFMA tiles per wave: a wm*tm*32 x wn*tn*32 tile
  int nst;             // LDS ring stages (halo: of the weight ring)
  int kp;              // tap gather, register-staged: k-tile depth BK; halo: patch rows PRMAX
  int opt;             // conv_halo_kernel's OPT
  int ksplit;
  int epi;             // the epilogue instantiated: EPI_PLAIN, or the bias form the shape takes
};
static const SplitWs kAnySplitWs{nullptr, nullptr, 1ll << 62, 1 << 30};  // planning only: every split-K plan fits

// Kernel family and tile of a forward (mode MODE_FWD) or 2-D dgrad call.  `ws`: the split-K workspace passed, if any.
// c64, then split-K, then the 64-row tiles of a small GEMM, then the halo tiles, then the tap gather by GEMM size;
// the register-staged gemm_nt_kernel for the stems' C = 4 / 1 and under avt_set_conv_variant(0).
static NtPlan plan_nt(const GemmNTParams& p, int mode, int epi, const SplitWs* ws) {
  const bool vid = p.IT > 1 || p.OT > 1 || p.KT > 1;
  const bool bias = epi != EPI_PLAIN;
  // a bias epilogue is instantiated on the Conv3d / long-tap-list argument form only for what needs it: a 2-D conv
  // of at most 9 taps takes the narrow form whichever entry point it came through
  if (bias) epi = vid || p.R * p.S > 9 ? EPI_BIAS3D : EPI_BIAS2D;
  // The canonical tile of a bias epilogue: the knobs that only trade ring depth or wave layout (halo stages, halo8
  // form / nst / tps2, AVT_C64_WAVES, the nt64 / nt128 tile overrides) stay at their defaults there -- they do not
  // change a result bit, and each would cost another instantiation.  Everything below reads them from here.
  const int nst128 = bias ? 2 : halo_nst(), nst64 = bias ? 3 : halo_small_nst();
  const int form8 = bias ? 0 : halo8_form(), nst8 = bias ? 3 : halo8_nst();
  const bool tps2 = !bias && halo_tps2();
  const int c64w = bias ? 8 : c64_waves();
  const int cfg64 = bias ? -1 : g_nt64_config, cfg128 = bias ? -1 : g_nt128_config;
  const auto ring = [](int nst) { return nst >= 3 && nst <= 5 ? nst : 2; };
  const auto tile = [epi](int family, int wm, int wn, int tm, int tn, int nst, int kp, int opt = 0, int ksplit = 1) {
    return NtPlan{family, wm, wn, tm, tn, nst, kp, opt, ksplit, epi};
  };

  if (!bias && mode == MODE_FWD && !vid && (p.IC == 4 || p.IC == 1) && stem_enabled() && p.Ng == 64 && p.R == 7 &&
      p.S == 7 && p.stride == 2 && p.pad == 3 && (p.IC == 4 ? stem_fits<4>(p.OW) : stem_fits<1>(p.OW)))
    return tile(NT_STEM, kStemNW, 1, 0, 0, 0, 0);  // conv_stem_fwd_kernel: kStemNW wave tiles per block
  if (p.IC % 32 != 0 || conv_variant() != 1)  // 128 x 128 or 128 x 64, double-buffered
    return tile(NT_REG, 2, 2, 2, p.IC % 32 == 0 && p.Ng % 128 == 0 ? 2 : 1, 2, 32);

  if (mode == MODE_FWD && halo3d_eligible(p)) {  // the three-patch form, 8 waves
    if (p.Ng == 64) return tile(NT_HALO3D, 8, 1, 1, 2, 3, 488, 4);                  // 256 x 64 on waves of 32 x 64
    if (!halo256_short(p)) return tile(NT_HALO3D, 4, 2, 2, 2, 2, kHaloPR, 4);       // W <= 79: 2 weight stages
    if (tps2 && halo_tps2_shape(p, 3)) return tile(NT_HALO3D, 4, 2, 2, 2, 2, 336, 7);  // two taps per barrier
    return tile(NT_HALO3D, 4, 2, 2, 2, 3, 336, 4);                                  // 256 x 128, W <= 39
  }
  if (c64_eligible(p)) return tile(NT_C64, c64w, 1, 0, 0, 0, c64::PRMAX);
  if (!bias && ws != nullptr && !vid) {
    const int ks = halo_splitk(p);
    const long long tiles = (long long)((p.M + 127) / 128) * (p.Ng / 128);
    // the plan is re-made at every call from the current knobs: a workspace sized for another plan
    // (the knobs changed after it was allocated) runs the shape without split-K rather than overrun it
    if (ks > 1 && tiles * ks * 128 * 128 <= ws->part_floats && tiles <= ws->counters)
      return tile(NT_HALO, 2, 2, 2, 2, ring(nst128), 168, 0, ks);
  }
  // (the tile overrides switch the 64-row tiles off under either epilogue: the live knobs, not the canonical ones)
  if (!vid && g_nt128_config < 0 && (g_nt64_config < 0 || g_nt64_config == 1) && p.bx == nullptr &&
      use_small_tile(p, p.Ng % 128 == 0 ? 128 : 64)) {
    if (p.Ng % 128 != 0) return tile(NT_GATHER, 2, 2, 1, 1, 3, 32);  // 64 x 64, k32, 3 stages
    if (halo_eligible(p) && 64 + 2 * p.OW + 2 <= 104) return tile(NT_HALO, 2, 2, 1, 2, ring(nst64), 104);  // 64 x 128
    return tile(NT_GATHER, 2, 2, 1, 2, 3, 32);  // 64 x 128, k32, 3 stages
  }
  if (halo_eligible(p)) {
    // measured (tools/conv_bench.py): the 4-wave 128 x 128 form at 2 blocks per CU beats the tap
    // gather on layer3/4 (W <= 19: +2..16 %); the 8-wave 256-row forms a patch of the wider layer1/2
    // images needs (1 block per CU) lose to it (-1..-20 %), so those keep the tap-gather kernel
    if (p.Ng % 128 == 0 && (g_halo == 2 || !halo128_fits(p) || halo8_pick(p))) {
      if (!halo256_short(p)) return tile(NT_HALO, 4, 2, 2, 2, 2, kHaloPR);  // W <= 79: 2 weight stages fit 416 rows
      if (form8 == 1) return tile(NT_HALO, 2, 2, 4, 2, 3, 336);  // same tile on 4 waves of 128 x 64
      if (nst8 == 4) return tile(NT_HALO, 4, 2, 2, 2, 4, 336);   // 4-stage weight ring: 150 KB of LDS, 1 block/CU
      if (tps2 && halo_tps2_shape(p)) return tile(NT_HALO, 4, 2, 2, 2, 2, 336, 3);  // two taps per barrier (layer4)
      return tile(NT_HALO, 4, 2, 2, 2, 3, 336);                  // 256 x 128, 8 waves, W <= 39 (layer2)
    }
    if (g_halo == 2) return tile(NT_HALO, 4, 2, 2, 1, 3, kHaloPR);  // 256 x 64, 8 waves (A/B only)
    // the 4-wave 128 x 128 tile by weight-ring depth (avt_set_halo_stages / AVT_HALO_NST): 2 stages (80 KB LDS, 2
    // blocks per CU; one 16 KiB weight stage in flight behind each step's 16 MFMAs per wave) or 3-5 (96-128 KB, 1
    // block per CU; NSTB-1 stages in flight)
    return tile(NT_HALO, 2, 2, 2, 2, ring(nst128), 168);
  }
  NtPlan g;
  if (p.Ng % 128 == 0) {
    // default: 256-row tiles (8 waves) where the GEMM is tall enough to fill the chip with them
    // (layer2, the stride-2 convs), 128 x 128 k64 tiles for the short layer3/4 GEMMs
    // Conv3d (27 taps: 3x the K of a 3x3) keeps the 128 x 128 k64 tile unless K is short: on the R3D-18
    // trunk (tools/conv3d_bench.py, profiles/r5_conv3d_tiles.txt) it is 10-15 % faster than the 256-row
    // form on layer2/3's 3x3x3 convs; at layer2.0's K = 1728 the two are within 3 %
    switch (cfg128 >= 0 ? cfg128 : (p.M >= 65536 && (!vid || p.Kg < 3072) ? 6 : 1)) {
      case 1: g = tile(NT_GATHER, 2, 2, 2, 2, 2, 64); break;   // 128 x 128, k64, 2 stages
      case 2: g = tile(NT_GATHER, 2, 2, 2, 2, 3, 64); break;   // 128 x 128, k64, 3 stages
      case 3: g = tile(NT_GATHER, 2, 2, 4, 2, 3, 32); break;   // 256 x 128, k32, 3 stages
      case 4: g = tile(NT_GATHER, 2, 2, 4, 2, 2, 64); break;   // 256 x 128, k64, 2 stages
      case 5: g = tile(NT_GATHER, 4, 2, 2, 2, 2, 64); break;   // 256 x 128, 8 waves, k64, 2 stages
      case 6: g = tile(NT_GATHER, 4, 2, 2, 2, 3, 32); break;   // 256 x 128, 8 waves, k32, 3 stages
      default: g = tile(NT_GATHER, 2, 2, 2, 2, 4, 32); break;  // 128 x 128, k32, 4 stages
    }
  } else {  // 64-wide N (layer1 / stem-fed convs)
    // auto (-1): 1, or 2 (4 stages) for a Conv3d -- R3D-18 layer1, profiles/r5_conv3d_tiles.txt: 548-579 us
    // against 557-683 us per conv, ahead in every ordering measured
    switch (cfg64 >= 0 ? cfg64 : (vid ? 2 : 1)) {
      case 0: g = tile(NT_GATHER, 4, 1, 2, 2, 4, 32); break;   // 256 x 64, 4 stages
      case 2: g = tile(NT_GATHER, 2, 2, 2, 1, 4, 32); break;   // 128 x 64, 4 stages
      case 3: g = tile(NT_GATHER, 4, 1, 2, 2, 2, 32); break;   // 256 x 64, 2 stages
      case 4: g = tile(NT_GATHER, 2, 2, 2, 1, 3, 64); break;   // 128 x 64, k64, 3 stages
      case 5: g = tile(NT_GATHER, 4, 1, 2, 2, 2, 64); break;   // 256 x 64, k64, 2 stages
      case 6: g = tile(NT_GATHER, 2, 2, 2, 1, 2, 64); break;   // 128 x 64, k64, 2 stages
      case 7: g = tile(NT_GATHER, 4, 2, 2, 1, 3, 64); break;   // 256 x 64, 8 waves, k64, 3 stages
      case 8: g = tile(NT_GATHER, 4, 2, 2, 1, 2, 64); break;   // 256 x 64, 8 waves, k64, 2 stages
      default: g = tile(NT_GATHER, 2, 2, 2, 1, 3, 32); break;  // 128 x 64, 3 stages
    }
  }
  // a 64-deep k-tile needs whole 64-channel taps: else the 4-wave k32 tile of the same width
  if (g.kp == 64 && p.IC % 64 != 0) g = tile(NT_GATHER, 2, 2, 2, g.wn * g.tn / 2, 3, 32);
  return g;
}

// Launches a plan.  Every launch_halo / launch_glds instantiation is named here, once; the bias epilogues (EPI) are
// instantiated for the tiles plan_nt can give them -- its canonical ones -- and the rest only for the plain epilogue.
// False: no such instantiation (a planner bug).
template <int MODE, int EPI = EPI_PLAIN>
static bool launch_plan(const NtPlan& pl, const GemmNTParams& p, hipStream_t st, const SplitWs* ws = nullptr) {
  constexpr bool PLAIN = EPI == EPI_PLAIN;
  float* part = pl.ksplit > 1 ? ws->part : nullptr;
  int* cnt = pl.ksplit > 1 ? ws->cnt : nullptr;
  const auto is = [&pl](int wm, int wn, int tm, int tn, int nst, int kp, int opt = 0) {
    return pl.wm == wm && pl.wn == wn && pl.tm == tm && pl.tn == tn && pl.nst == nst && pl.kp == kp && pl.opt == opt;
  };
#define AVT_HALO(WM, WN, TM, TN, NST, PR, OPT)                                              \
  if (is(WM, WN, TM, TN, NST, PR, OPT)) {                                                   \
    launch_halo<MODE, WM, WN, TM, TN, NST, PR, OPT, !PLAIN>(p, st, pl.ksplit, part, cnt);   \
    return true;                                                                            \
  }
#define AVT_GLDS(WM, WN, TM, TN, NST, BK)                     \
  if (is(WM, WN, TM, TN, NST, BK)) {                                \
    return launch_glds<MODE, WM, WN, TM, TN, NST, BK, EPI>(p, st);  \
  }
  switch (pl.family) {
    case NT_C64:
      if constexpr (EPI != EPI_BIAS3D) {
        launch_c64<MODE, !PLAIN>(p, st, pl.wm);
        return true;
      }
      break;
    case NT_HALO:
      if constexpr (EPI != EPI_BIAS3D) {
        AVT_HALO(2, 2, 1, 2, 3, 104, 0)      // 64 x 128
        AVT_HALO(2, 2, 2, 2, 2, 168, 0)      // 128 x 128
        AVT_HALO(4, 2, 2, 2, 3, 336, 0)      // 256 x 128, W <= 39
        AVT_HALO(4, 2, 2, 2, 2, kHaloPR, 0)  // 256 x 128, W <= 79
        AVT_HALO(4, 2, 2, 1, 3, kHaloPR, 0)  // 256 x 64
      }
      if constexpr (PLAIN) {  // avt_set_halo_stages, avt_set_halo8_form / _nst, avt_set_halo_tps2
        AVT_HALO(2, 2, 1, 2, 2, 104, 0)
        AVT_HALO(2, 2, 1, 2, 4, 104, 0)
        AVT_HALO(2, 2, 1, 2, 5, 104, 0)
        AVT_HALO(2, 2, 2, 2, 3, 168, 0)
        AVT_HALO(2, 2, 2, 2, 4, 168, 0)
        AVT_HALO(2, 2, 2, 2, 5, 168, 0)
        AVT_HALO(2, 2, 4, 2, 3, 336, 0)
        AVT_HALO(4, 2, 2, 2, 4, 336, 0)
        AVT_HALO(4, 2, 2, 2, 2, 336, 3)
      }
      break;
    case NT_HALO3D:  // OPT 4: the Conv3d 3x3x3 / stride 1 / pad 1 form (conv_halo.h; forward only)
      if constexpr (MODE == MODE_FWD && EPI != EPI_BIAS2D) {
        AVT_HALO(8, 1, 1, 2, 3, 488, 4)
        AVT_HALO(4, 2, 2, 2, 3, 336, 4)
        AVT_HALO(4, 2, 2, 2, 2, kHaloPR, 4)
        if constexpr (PLAIN) AVT_HALO(4, 2, 2, 2, 2, 336, 7)  // avt_set_halo_tps2
      }
      break;
    case NT_GATHER:
      AVT_GLDS(2, 2, 1, 1, 3, 32)
      AVT_GLDS(2, 2, 1, 2, 3, 32)
      AVT_GLDS(2, 2, 2, 1, 3, 32)
      AVT_GLDS(2, 2, 2, 2, 2, 64)
      AVT_GLDS(2, 2, 2, 2, 3, 32)
      AVT_GLDS(4, 2, 2, 2, 3, 32)
      if constexpr (EPI != EPI_BIAS2D) AVT_GLDS(2, 2, 2, 1, 4, 32)  // a Conv3d's 64-wide tile
      if constexpr (PLAIN) {  // avt_set_nt128_config, avt_set_nt64_config
        AVT_GLDS(2, 2, 2, 2, 4, 32)
        AVT_GLDS(2, 2, 2, 2, 3, 64)
        AVT_GLDS(2, 2, 4, 2, 3, 32)
        AVT_GLDS(2, 2, 4, 2, 2, 64)
        AVT_GLDS(4, 2, 2, 2, 2, 64)
        AVT_GLDS(4, 1, 2, 2, 4, 32)
        AVT_GLDS(4, 1, 2, 2, 2, 32)
        AVT_GLDS(2, 2, 2, 1, 3, 64)
        AVT_GLDS(4, 1, 2, 2, 2, 64)
        AVT_GLDS(2, 2, 2, 1, 2, 64)
        AVT_GLDS(4, 2, 2, 1, 3, 64)
        AVT_GLDS(4, 2, 2, 1, 2, 64)
      }
      break;
    case NT_REG:
      if constexpr (PLAIN) {
        const dim3 grid(((p.M + 127) / 128) * (p.Ng / (64 * pl.tn)));
        if (p.IC % 32 == 0 && pl.tn == 2)
          hipLaunchKernelGGL((gemm_nt_kernel<MODE, 8, 128, 128>), grid, dim3(256), 0, st, p);
        else if (p.IC % 32 == 0)
          hipLaunchKernelGGL((gemm_nt_kernel<MODE, 8, 128, 64>), grid, dim3(256), 0, st, p);
        else if constexpr (MODE == MODE_FWD) {  // the stems
          if (p.IC == 4)
            hipLaunchKernelGGL((gemm_nt_kernel<MODE, 4, 128, 64>), grid, dim3(256), 0, st, p);
          else
            hipLaunchKernelGGL((gemm_nt_kernel<MODE, 1, 128, 64>), grid, dim3(256), 0, st, p);
        } else {
          break;
        }
        return true;
      }
      break;
  }
#undef AVT_HALO
#undef AVT_GLDS
  return false;
}

// The forward GemmNTParams of a conv (a 2-D conv: T = KT = 1, pad_t = 0); the caller adds its epilogue operands.
// False: an activation tensor reaches 2 GiB (the kernels' 32-bit buffer offsets).
static bool fwd_params(GemmNTParams& p, const void* x, const void* wpack, void* y, int N, int T, int H, int W, int Cp,
                       int K, int KT, int R, int S, int stride, int pad_t, int pad, int Kg) {
  p.act = (const bf16_t*)x;
  p.wmat = (const bf16_t*)wpack;
  p.out = (bf16_t*)y;
  p.IT = T; p.IH = H; p.IW = W; p.IC = Cp;
  p.OT = T + 2 * pad_t - KT + 1;
  p.OH = conv_out(H, R, stride, pad);
  p.OW = conv_out(W, S, stride, pad);
  p.M = N * p.OT * p.OH * p.OW;
  p.Ng = K;
  p.Kg = Kg;
  p.KT = KT; p.R = R; p.S = S; p.stride = stride; p.pad = pad; p.pad_t = pad_t;
  return (size_t)N * T * H * W * Cp * 2 < (1ull << 31) && (size_t)N * p.OT * p.OH * p.OW * K * 2 < (1ull << 31);
}

// One of the two bias epilogues' launches (plan_nt resolves which)
static bool launch_plan_bias(const NtPlan& pl, const GemmNTParams& p, hipStream_t st) {
  return pl.epi == EPI_BIAS2D ? launch_plan<MODE_FWD, EPI_BIAS2D>(pl, p, st) : launch_plan<MODE_FWD, EPI_BIAS3D>(pl, p, st);
}

static int conv2d_fwd_impl(const void* x, const void* wpack, void* y, double* bn_acc, int N, int H, int W, int Cp,
                           int K, int R, int S, int stride, int pad, int Kg, const SplitWs* ws, void* stream);

extern "C" int avt_conv2d_fwd(const void* x, const void* wpack, void* y, double* bn_acc, int N, int H, int W,
                              int Cp, int K, int R, int S, int stride, int pad, int Kg, void* stream) {
  return conv2d_fwd_impl(x, wpack, y, bn_acc, N, H, W, Cp, K, R, S, stride, pad, Kg, nullptr, stream);
}

// split-K workspace of a 3x3/s1 conv (halo kernel): *part_floats fp32 partials, *counters ints (zero
// before the first launch; the kernel leaves them zero).  Both 0: the shape runs without split-K.
extern "C" int avt_conv2d_splitk_plan(int N, int H, int W, int C, int K, int R, int S, int stride, int pad, int dgrad,
                                      long long* part_floats, int* counters) {
  AVT_REQUIRE(part_floats && counters, "conv2d_splitk_plan: null pointer");
  *part_floats = 0;
  *counters = 0;
  GemmNTParams p{};
  p.IT = p.OT = p.KT = 1;
  p.R = R; p.S = S; p.stride = stride; p.pad = pad;
  if (dgrad) {
    p.IH = conv_out(H, R, stride, pad); p.IW = conv_out(W, S, stride, pad); p.IC = K;
    p.OH = H; p.OW = W; p.Ng = C;
  } else {
    p.IH = H; p.IW = W; p.IC = C;
    p.OH = conv_out(H, R, stride, pad); p.OW = conv_out(W, S, stride, pad); p.Ng = K;
  }
  p.M = N * p.OH * p.OW;
  if (p.IC % 64 != 0 || p.Ng % 64 != 0 || p.M <= 0) return AVT_OK;
  const int ks = plan_nt(p, dgrad ? MODE_DGRAD : MODE_FWD, EPI_PLAIN, &kAnySplitWs).ksplit;
  if (ks <= 1) return AVT_OK;
  const int tiles = ((p.M + 127) / 128) * (p.Ng / 128);
  *part_floats = (long long)tiles * ks * 128 * 128;
  *counters = tiles;
  return AVT_OK;
}

extern "C" int avt_set_halo8_nst(int nst) {
  AVT_REQUIRE(nst == -1 || nst == 3 || nst == 4, "set_halo8_nst: -1, 3 or 4");
  avt::g_halo8_nst = nst;  // -1: back to the environment default
  return AVT_OK;
}

extern "C" int avt_set_halo8_form(int form) {
  AVT_REQUIRE(form >= -1 && form <= 1, "set_halo8_form: -1, 0 or 1");
  avt::g_halo8_form = form;  // -1: back to the environment default
  return AVT_OK;
}

extern "C" int avt_set_halo_splitk(int ksplit, int target_blocks) {
  AVT_REQUIRE(ksplit >= 0 && target_blocks >= 0, "set_halo_splitk: bad arguments");
  g_halo_splitk = ksplit;
  g_splitk_blocks = target_blocks > 0 ? target_blocks : 2 * num_cus();
  return AVT_OK;
}

extern "C" int avt_conv2d_fwd_ws(const void* x, const void* wpack, void* y, double* bn_acc, int N, int H, int W,
                                 int Cp, int K, int R, int S, int stride, int pad, int Kg, float* part,
                                 long long part_floats, int* cnt, int counters, void* stream) {
  AVT_REQUIRE(part_floats >= 0 && counters >= 0, "conv2d_fwd_ws: negative workspace size");
  const SplitWs ws{part, cnt, part_floats, counters};
  return conv2d_fwd_impl(x, wpack, y, bn_acc, N, H, W, Cp, K, R, S, stride, pad, Kg, (part && cnt) ? &ws : nullptr,
                         stream);
}

static int conv2d_fwd_impl(const void* x, const void* wpack, void* y, double* bn_acc, int N, int H, int W, int Cp,
                           int K, int R, int S, int stride, int pad, int Kg, const SplitWs* ws, void* stream) {
  AVT_REQUIRE(x && wpack && y, "conv2d_fwd: null pointer");
  AVT_REQUIRE(K % 64 == 0, "conv2d_fwd: K=%d must be a multiple of 64", K);
  AVT_REQUIRE(Kg % 32 == 0 && Kg >= R * S * Cp, "conv2d_fwd: Kg=%d must be a multiple of 32 >= R*S*C", Kg);
  AVT_REQUIRE(Cp % 32 == 0 || Cp == 4 || Cp == 1, "conv2d_fwd: C=%d unsupported (need %%32, or stem 1/4)", Cp);
  AVT_REQUIRE(Cp % 32 != 0 || Kg == R * S * Cp, "conv2d_fwd: Kg must equal R*S*C for C%%32==0");
  AVT_REQUIRE(Cp % 32 != 0 || R * S <= kMaxTaps, "conv2d_fwd: at most %d taps for C%%32==0", kMaxTaps);
  AVT_REQUIRE(stride == 1 || stride == 2, "conv2d_fwd: stride must be 1 or 2");
  AVT_REQUIRE(N >= 1 && H >= 1 && W >= 1 && R >= 1 && S >= 1 && pad >= 0 && H + 2 * pad >= R && W + 2 * pad >= S,
              "conv2d_fwd: empty input, taps or output, or negative padding");
  GemmNTParams p{};
  AVT_REQUIRE(fwd_params(p, x, wpack, y, N, 1, H, W, Cp, K, 1, R, S, stride, 0, pad, Kg),
              "conv2d_fwd: activation tensors must stay below 2 GiB (32-bit buffer offsets)");
  p.stats = bn_acc;
  hipStream_t st = (hipStream_t)stream;
  const NtPlan pl = plan_nt(p, MODE_FWD, EPI_PLAIN, ws);
  if (pl.family == NT_STEM) {
    StemArgs sa{};
    sa.x = p.act;
    sa.w = p.wmat;
    sa.y = p.out;
    sa.stats = bn_acc;
    sa.x_bytes = (unsigned)((size_t)N * H * W * Cp * 2);
    sa.y_bytes = (unsigned)((size_t)p.M * K * 2);
    sa.N = N;
    sa.IH = H; sa.IW = W; sa.OH = p.OH; sa.OW = p.OW; sa.Kg = Kg;
    sa.tiles_per_row = (p.OW + 31) / 32;
    sa.total_tiles = N * p.OH * sa.tiles_per_row;
    const int blocks = (sa.total_tiles + kStemNW - 1) / kStemNW;  // kStemNW wave tiles per block round
    const int grid = blocks < num_cus() ? blocks : num_cus();
    const size_t lds = Cp == 4 ? stem_lds_bytes<4>() : stem_lds_bytes<1>();
    if (Cp == 4)
      hipLaunchKernelGGL(conv_stem_fwd_kernel<4>, dim3(grid), dim3(kStemNW * 64), lds, st, sa);
    else
      hipLaunchKernelGGL(conv_stem_fwd_kernel<1>, dim3(grid), dim3(kStemNW * 64), lds, st, sa);
    return check_launch("conv2d_fwd (stem)");
  }
  AVT_REQUIRE(launch_plan<MODE_FWD>(pl, p, st, ws), "conv2d_fwd: no kernel for the plan");
  return check_launch("conv2d_fwd");
}

// Forward conv with BatchNorm folded in (include/avt.h): y = [relu](conv(x, wpack) + bias[k] (+ residual)).
extern "C" int avt_conv2d_fwd_bias(const void* x, const void* wpack, void* y, int N, int H, int W, int Cp, int K,
                                   int R, int S, int stride, int pad, int Kg, const float* bias, const void* residual,
                                   int relu, void* stream) {
  AVT_REQUIRE(x && wpack && y, "conv2d_fwd_bias: null pointer");
  AVT_REQUIRE(bias, "conv2d_fwd_bias: bias is required (avt_conv2d_fwd is the conv without one)");
  AVT_REQUIRE(residual == nullptr || residual != y, "conv2d_fwd_bias: residual must not alias y");
  AVT_REQUIRE(N >= 1 && H >= 1 && W >= 1, "conv2d_fwd_bias: empty input");
  AVT_REQUIRE(K >= 64 && K % 64 == 0, "conv2d_fwd_bias: K=%d must be a multiple of 64", K);
  AVT_REQUIRE(Cp >= 32 && Cp % 32 == 0, "conv2d_fwd_bias: C=%d must be a multiple of 32 (the stems keep avt_conv2d_fwd)", Cp);
  AVT_REQUIRE(R >= 1 && S >= 1 && R * S <= 9, "conv2d_fwd_bias: at most 9 taps");
  AVT_REQUIRE(Kg == R * S * Cp, "conv2d_fwd_bias: Kg=%d must equal R*S*C", Kg);
  AVT_REQUIRE(stride == 1 || stride == 2, "conv2d_fwd_bias: stride must be 1 or 2");
  AVT_REQUIRE(pad >= 0 && H + 2 * pad >= R && W + 2 * pad >= S, "conv2d_fwd_bias: empty output");
  AVT_REQUIRE(conv_variant() == 1, "conv2d_fwd_bias: needs the LDS-DMA conv kernels (AVT_CONV_VARIANT=1)");
  GemmNTParams p{};
  AVT_REQUIRE(fwd_params(p, x, wpack, y, N, 1, H, W, Cp, K, 1, R, S, stride, 0, pad, Kg),
              "conv2d_fwd_bias: activation tensors must stay below 2 GiB (32-bit buffer offsets)");
  p.add = (const bf16_t*)residual;
  p.bias = bias;
  p.relu = relu ? 1 : 0;
  AVT_REQUIRE(launch_plan_bias(plan_nt(p, MODE_FWD, EPI_BIAS2D, nullptr), p, (hipStream_t)stream),
              "conv2d_fwd_bias: no kernel for the plan");
  return check_launch("conv2d_fwd_bias");
}

static int conv2d_dgrad_impl(const void* dy, const void* wt, void* dx, const void* add, const void* add_mask, int N,
                             int H, int W, int C, int K, int R, int S, int stride, int pad, const avt_dgrad_bn_epi* epi,
                             void* stream, const SplitWs* ws = nullptr) {
  AVT_REQUIRE(dy && wt && dx, "conv2d_dgrad: null pointer");
  AVT_REQUIRE(epi == nullptr || (epi->xc && epi->stats && epi->acc), "conv2d_dgrad: epilogue needs xc, stats, acc");
  AVT_REQUIRE(epi == nullptr || epi->xc2 == nullptr || (epi->stats2 && epi->acc2),
              "conv2d_dgrad: second BN needs stats2 and acc2");
  AVT_REQUIRE(epi == nullptr || ((uintptr_t)epi->acc & 7) == 0, "conv2d_dgrad: acc must be 8-byte aligned");
  // only the LDS-DMA kernels write the epilogue's slots and header; the register-staged gemm_nt_kernel ignores it
  AVT_REQUIRE(epi == nullptr || conv_variant() == 1,
              "conv2d_dgrad: the BatchNorm-backward epilogue needs the LDS-DMA kernels (avt_set_conv_variant(1))");
  AVT_REQUIRE(C % 64 == 0 && K % 32 == 0, "conv2d_dgrad: C=%d K=%d unsupported", C, K);
  AVT_REQUIRE(stride == 1 || stride == 2, "conv2d_dgrad: stride must be 1 or 2");
  AVT_REQUIRE(R >= 1 && S >= 1 && R * S <= 32, "conv2d_dgrad: at most 32 taps");
  // one launch walks at most 9 taps (the 2-D kernels' argument block): all R*S at stride 1, a parity class's at 2
  AVT_REQUIRE((stride == 1 ? R * S : ((R + 1) / 2) * ((S + 1) / 2)) <= 9,
              "conv2d_dgrad: at most 9 taps per launch (R*S at stride 1, ceil(R/2)*ceil(S/2) at stride 2), got %dx%d",
              R, S);
  // (a tap list of pad - r, pad - s displacements: the same bound avt_conv3d_dgrad puts on its padding)
  AVT_REQUIRE(pad >= 0 && pad < R && pad < S, "conv2d_dgrad: padding must be below the kernel size");
  AVT_REQUIRE(N >= 1 && H >= 1 && W >= 1 && H + 2 * pad >= R && W + 2 * pad >= S, "conv2d_dgrad: empty gradient");
  GemmNTParams p{};
  p.act = (const bf16_t*)dy;
  p.wmat = (const bf16_t*)wt;
  p.out = (bf16_t*)dx;
  p.add = (const bf16_t*)add;
  p.amask = (const unsigned char*)add_mask;
  p.stats = nullptr;
  p.IH = conv_out(H, R, stride, pad);
  p.IW = conv_out(W, S, stride, pad);
  p.IC = K;
  p.OH = H; p.OW = W;
  p.IT = p.OT = p.KT = 1;
  p.pad_t = 0;
  p.M = N * H * W;
  AVT_REQUIRE((size_t)p.M * C * 2 < (1ull << 31) && (size_t)N * p.IH * p.IW * K * 2 < (1ull << 31),
              "conv2d_dgrad: activation tensors must stay below 2 GiB (32-bit buffer offsets)");
  p.Ng = C;
  p.Kg = R * S * K;
  p.R = R; p.S = S; p.stride = stride; p.pad = pad;
  if (epi != nullptr) {
    p.bx = (const bf16_t*)epi->xc;
    p.by = (const bf16_t*)epi->y;
    p.bst = epi->stats;
    p.bacc = epi->acc;
    p.bx2 = (const bf16_t*)epi->xc2;
    p.bst2 = epi->stats2;
    p.bacc2 = epi->acc2;
    p.bskip00 = epi->skip_class00;
    p.bappend = epi->append_slots ? 1 : 0;
  }
  AVT_REQUIRE(launch_plan<MODE_DGRAD>(plan_nt(p, MODE_DGRAD, EPI_PLAIN, ws), p, (hipStream_t)stream, ws),
              "conv2d_dgrad: no kernel for the plan");
  return check_launch("conv2d_dgrad");
}

// avt_conv2d_dgrad / avt_conv2d_dgrad_mask (add_mask optional) with a split-K workspace
extern "C" int avt_conv2d_dgrad_ws(const void* dy, const void* wt, void* dx, const void* add, const void* add_mask,
                                   int N, int H, int W, int C, int K, int R, int S, int stride, int pad, float* part,
                                   long long part_floats, int* cnt, int counters, void* stream) {
  AVT_REQUIRE(add_mask == nullptr || (add && add != dx), "conv2d_dgrad_ws: add_mask needs add, not aliasing dx");
  AVT_REQUIRE(part_floats >= 0 && counters >= 0, "conv2d_dgrad_ws: negative workspace size");
  const SplitWs ws{part, cnt, part_floats, counters};
  return conv2d_dgrad_impl(dy, wt, dx, add, add_mask, N, H, W, C, K, R, S, stride, pad, nullptr, stream,
                           (part && cnt) ? &ws : nullptr);
}

extern "C" int avt_conv2d_dgrad_bn(const void* dy, const void* wt, void* dx, const void* add, int N, int H, int W,
                                   int C, int K, int R, int S, int stride, int pad, const avt_dgrad_bn_epi* epi,
                                   void* stream) {
  return conv2d_dgrad_impl(dy, wt, dx, add, nullptr, N, H, W, C, K, R, S, stride, pad, epi, stream);
}

extern "C" int avt_conv2d_dgrad(const void* dy, const void* wt, void* dx, const void* add, int N, int H, int W, int C,
                                int K, int R, int S, int stride, int pad, void* stream) {
  return conv2d_dgrad_impl(dy, wt, dx, add, nullptr, N, H, W, C, K, R, S, stride, pad, nullptr, stream);
}

extern "C" int avt_conv2d_dgrad_mask(const void* dy, const void* wt, void* dx, const void* add, const void* add_mask,
                                     int N, int H, int W, int C, int K, int R, int S, int stride, int pad,
                                     void* stream) {
  AVT_REQUIRE(add && add_mask, "conv2d_dgrad_mask: add and add_mask are required");
  AVT_REQUIRE(add != dx, "conv2d_dgrad_mask: add must not alias dx");
  return conv2d_dgrad_impl(dy, wt, dx, add, add_mask, N, H, W, C, K, R, S, stride, pad, nullptr, stream);
}

// Conv3d forward (the R3D-18 video trunk, models/resnet3D.py:14-28 conv3x3x3 / conv1x1x1, called
// from BasicBlock.forward 45-61): x NDHWC bf16 [N][T][H][W][Cp], wpack bf16 [K][(kt,r,s,c)],
// y NDHWC bf16 [N][T'][H'][W'][K] with T' = T + 2*pad_t - KT + 1 (temporal stride 1, as every
// Conv3d of the R3D-18 built by model.py:20 after the stem) and spatial stride `stride`.
// BN statistics are accumulated in the epilogue exactly as conv2d_fwd.
// (`add`: optional [N][T'][H'][W'][K] bf16 added in the store epilogue, may alias y -- avt_conv3d_dgrad's residual)
static int conv3d_fwd_impl(const void* x, const void* wpack, void* y, double* bn_acc, const void* add, int N, int T,
                           int H, int W, int Cp, int K, int KT, int R, int S, int stride, int pad_t, int pad,
                           void* stream) {
  AVT_REQUIRE(x && wpack && y, "conv3d_fwd: null pointer");
  AVT_REQUIRE(K % 64 == 0, "conv3d_fwd: K=%d must be a multiple of 64", K);
  AVT_REQUIRE(Cp % 32 == 0, "conv3d_fwd: C=%d must be a multiple of 32", Cp);
  AVT_REQUIRE(KT * R * S <= kMaxTaps && KT >= 1 && R >= 1 && S >= 1, "conv3d_fwd: at most %d taps", kMaxTaps);
  AVT_REQUIRE(stride == 1 || stride == 2, "conv3d_fwd: spatial stride must be 1 or 2");
  GemmNTParams p{};
  const bool fits = fwd_params(p, x, wpack, y, N, T, H, W, Cp, K, KT, R, S, stride, pad_t, pad, KT * R * S * Cp);
  AVT_REQUIRE(p.OT >= 1 && p.OH >= 1 && p.OW >= 1, "conv3d_fwd: empty output");
  AVT_REQUIRE(fits, "conv3d_fwd: activation tensors must stay below 2 GiB (32-bit buffer offsets)");
  AVT_REQUIRE(conv_variant() == 1, "conv3d_fwd: needs the LDS-DMA conv kernels (AVT_CONV_VARIANT=1)");
  p.add = (const bf16_t*)add;
  p.stats = bn_acc;
  AVT_REQUIRE(launch_plan<MODE_FWD>(plan_nt(p, MODE_FWD, EPI_PLAIN, nullptr), p, (hipStream_t)stream),
              "conv3d_fwd: no kernel for the plan");
  return check_launch("conv3d_fwd");
}

extern "C" int avt_conv3d_fwd(const void* x, const void* wpack, void* y, double* bn_acc, int N, int T, int H, int W,
                              int Cp, int K, int KT, int R, int S, int stride, int pad_t, int pad, void* stream) {
  return conv3d_fwd_impl(x, wpack, y, bn_acc, nullptr, N, T, H, W, Cp, K, KT, R, S, stride, pad_t, pad, stream);
}

// Conv3d forward with BatchNorm folded in (include/avt.h): y = [relu](conv3d(x, wpack) + bias[k] (+ residual)).
extern "C" int avt_conv3d_fwd_bias(const void* x, const void* wpack, void* y, int N, int T, int H, int W, int Cp,
                                   int K, int KT, int R, int S, int stride, int pad_t, int pad, const float* bias,
                                   const void* residual, int relu, void* stream) {
  AVT_REQUIRE(x && wpack && y, "conv3d_fwd_bias: null pointer");
  AVT_REQUIRE(bias, "conv3d_fwd_bias: bias is required (avt_conv3d_fwd is the conv without one)");
  AVT_REQUIRE(residual == nullptr || residual != y, "conv3d_fwd_bias: residual must not alias y");
  AVT_REQUIRE(N >= 1 && T >= 1 && H >= 1 && W >= 1, "conv3d_fwd_bias: empty input");
  AVT_REQUIRE(K >= 64 && K % 64 == 0, "conv3d_fwd_bias: K=%d must be a multiple of 64", K);
  AVT_REQUIRE(Cp >= 32 && Cp % 32 == 0, "conv3d_fwd_bias: C=%d must be a multiple of 32", Cp);
  AVT_REQUIRE(KT >= 1 && R >= 1 && S >= 1 && KT * R * S <= kMaxTaps, "conv3d_fwd_bias: at most %d taps", kMaxTaps);
  AVT_REQUIRE(stride == 1 || stride == 2, "conv3d_fwd_bias: spatial stride must be 1 or 2");
  AVT_REQUIRE(pad_t >= 0 && pad >= 0, "conv3d_fwd_bias: negative padding");
  AVT_REQUIRE(conv_variant() == 1, "conv3d_fwd_bias: needs the LDS-DMA conv kernels (AVT_CONV_VARIANT=1)");
  GemmNTParams p{};
  const bool fits = fwd_params(p, x, wpack, y, N, T, H, W, Cp, K, KT, R, S, stride, pad_t, pad, KT * R * S * Cp);
  AVT_REQUIRE(p.OT >= 1 && H + 2 * pad >= R && W + 2 * pad >= S, "conv3d_fwd_bias: empty output");
  AVT_REQUIRE(fits, "conv3d_fwd_bias: activation tensors must stay below 2 GiB (32-bit buffer offsets)");
  p.add = (const bf16_t*)residual;
  p.bias = bias;
  p.relu = relu ? 1 : 0;
  AVT_REQUIRE(launch_plan_bias(plan_nt(p, MODE_FWD, EPI_BIAS3D, nullptr), p, (hipStream_t)stream),
              "conv3d_fwd_bias: no kernel for the plan");
  return check_launch("conv3d_fwd_bias");
}

// The plan of a forward call, from its shape and the current knobs alone (include/avt_tuning.h): no GPU, no launch.
extern "C" int avt_conv_fwd_plan(int N, int T, int H, int W, int Cp, int K, int KT, int R, int S, int stride, int pad_t,
                                 int pad, int epi, int* plan) {
  AVT_REQUIRE(plan, "conv_fwd_plan: null pointer");
  AVT_REQUIRE(epi >= 0 && epi <= 3, "conv_fwd_plan: epi=%d (0 plain, 1 / 2 the 2-D / 3-D bias entry, 3 plain with a workspace)", epi);
  const bool bias = epi == EPI_BIAS2D || epi == EPI_BIAS3D;
  AVT_REQUIRE(N >= 1 && T >= 1 && H >= 1 && W >= 1 && KT >= 1 && R >= 1 && S >= 1 && pad_t >= 0 && pad >= 0,
              "conv_fwd_plan: empty input or taps, or negative padding");
  AVT_REQUIRE(K >= 64 && K % 64 == 0, "conv_fwd_plan: K=%d must be a multiple of 64", K);
  AVT_REQUIRE((Cp >= 32 && Cp % 32 == 0) || (!bias && T == 1 && KT == 1 && (Cp == 4 || Cp == 1)),
              "conv_fwd_plan: C=%d unsupported (need %%32, or a plain 2-D stem's 1/4)", Cp);
  AVT_REQUIRE(KT * R * S <= kMaxTaps || Cp % 32 != 0, "conv_fwd_plan: at most %d taps", kMaxTaps);
  AVT_REQUIRE(stride == 1 || stride == 2, "conv_fwd_plan: stride must be 1 or 2");
  AVT_REQUIRE(!bias || conv_variant() == 1, "conv_fwd_plan: the bias epilogues need the LDS-DMA conv kernels");
  GemmNTParams p{};
  const bool fits = fwd_params(p, nullptr, nullptr, nullptr, N, T, H, W, Cp, K, KT, R, S, stride, pad_t, pad,
                               (KT * R * S * Cp + 31) / 32 * 32);
  AVT_REQUIRE(p.OT >= 1 && p.OH >= 1 && p.OW >= 1, "conv_fwd_plan: empty output");
  AVT_REQUIRE(fits, "conv_fwd_plan: activation tensors must stay below 2 GiB (32-bit buffer offsets)");
  const NtPlan pl = plan_nt(p, MODE_FWD, epi == 3 ? EPI_PLAIN : epi, epi == 3 ? &kAnySplitWs : nullptr);
  const int out[AVT_CONV_PLAN_INTS] = {pl.family, pl.wm, pl.wn, pl.tm, pl.tn, pl.nst, pl.kp, pl.opt, pl.ksplit, pl.epi};
  for (int i = 0; i < AVT_CONV_PLAN_INTS; ++i) plan[i] = out[i];
  return AVT_OK;
}

// One parity class (ph, pw) of a spatially strided Conv3d's input gradient on the tap-gather kernel's Conv3d form:
// the 2-D class scheme (launch_glds) with the temporal taps -- the rows are the class's pixels (2h'+ph, 2w'+pw) of
// every frame, the K loop walks the class's spatial taps times all KT temporal taps (3x3 / pad 1 / stride 2: 1, 2, 2
// and 4 spatial taps), and the tap mask drops the frames outside the row's clip.  wt is the flipped pack of
// avt_pack_conv3d_weight_dgrad: tap (kt, r, s) is stored at (KT-1-kt, R-1-r, S-1-s).
template <int TN>
static void launch_dgrad3d_class(const GemmNTParams& p, int ph, int pw, hipStream_t st) {
  constexpr int BM = 128, BN = 64 * TN;
  NTPipeArgsV ta{};
  const int batch = p.M / (p.OT * p.OH * p.OW);  // clips
  ta.act_bytes = (unsigned)((size_t)batch * p.IT * p.IH * p.IW * p.IC * 2);
  ta.w_bytes = (unsigned)((size_t)p.Ng * p.Kg * 2);
  ta.cls = 1;
  ta.OHf = p.OH;
  ta.OWf = p.OW;
  ta.ph = ph;
  ta.pw = pw;
  for (int kt = 0; kt < p.KT; ++kt)
    for (int r = 0; r < p.R; ++r)
      for (int s = 0; s < p.S; ++s) {
        if (((ph + p.pad - r) & 1) || ((pw + p.pad - s) & 1)) continue;
        ta.tap_w[ta.ntaps] = ((p.KT - 1 - kt) * p.R + (p.R - 1 - r)) * p.S + (p.S - 1 - s);
        ta.tap_dt[ta.ntaps] = p.pad_t - kt;
        ta.tap_dy[ta.ntaps] = (ph + p.pad - r) / 2;
        ta.tap_dx[ta.ntaps] = (pw + p.pad - s) / 2;
        ++ta.ntaps;
      }
  GemmNTParams pc = p;
  pc.OH = (p.OH - ph + 1) / 2;
  pc.OW = (p.OW - pw + 1) / 2;
  pc.M = batch * p.OT * pc.OH * pc.OW;
  // a class no tap reaches is written as 0 (+ add) by an empty K loop; accumulating in place it is already final
  if (pc.M <= 0 || (ta.ntaps == 0 && p.add != nullptr && p.add == p.out)) return;
  ta.div_hw = make_magic((unsigned)(pc.OH * pc.OW));
  ta.div_ow = make_magic((unsigned)pc.OW);
  for (int k = 0; k < 4; ++k) ta.cdiv_hw[k] = ta.cdiv_ow[k] = make_magic(1u);
  const int grid = ((pc.M + BM - 1) / BM) * (p.Ng / BN);
  hipLaunchKernelGGL((conv_nt_pipe_kernel<MODE_DGRAD, 2, 2, 2, TN, 4, 32, true>), dim3(grid), dim3(256), 0, st, pc, ta);
}

// Conv3d input gradient (autograd's backward of conv3x3x3, models/resnet3D.py:14-20, in BasicBlock.forward 45-61):
// dx[N][T][H][W][C] = dgrad(dy[N][T][P][Q][K], wt[C][(KT-1-kt, R-1-r, S-1-s, k)]) (+ add, which may alias dx).
// Spatial stride 1: the forward conv of dy with the flipped, (K, C)-transposed weights and pad' = k - 1 - pad, on
// avt_conv3d_fwd's own launch path (the three-patch halo form included).  Stride 2: the four parity classes above.
extern "C" int avt_conv3d_dgrad(const void* dy, const void* wt, void* dx, const void* add, int N, int T, int H, int W,
                                int C, int K, int KT, int R, int S, int stride, int pad_t, int pad, void* stream) {
  AVT_REQUIRE(dy && wt && dx, "conv3d_dgrad: null pointer");
  AVT_REQUIRE(C % 64 == 0 && K % 32 == 0, "conv3d_dgrad: C=%d (a multiple of 64) K=%d (of 32) unsupported", C, K);
  AVT_REQUIRE(KT >= 1 && R >= 1 && S >= 1 && KT * R * S <= kMaxTaps, "conv3d_dgrad: at most %d taps", kMaxTaps);
  AVT_REQUIRE(stride == 1 || stride == 2, "conv3d_dgrad: spatial stride must be 1 or 2");
  AVT_REQUIRE(pad_t >= 0 && pad >= 0 && pad_t < KT && pad < R && pad < S, "conv3d_dgrad: padding must be below the kernel size");
  const int To = T + 2 * pad_t - KT + 1, P = conv_out(H, R, stride, pad), Q = conv_out(W, S, stride, pad);
  AVT_REQUIRE(N >= 1 && To >= 1 && P >= 1 && Q >= 1, "conv3d_dgrad: empty gradient");
  if (stride == 1) {
    AVT_REQUIRE(R == S, "conv3d_dgrad: square spatial taps only");
    return conv3d_fwd_impl(dy, wt, dx, nullptr, add, N, To, P, Q, K, C, KT, R, S, 1, KT - 1 - pad_t, R - 1 - pad,
                           stream);
  }
  AVT_REQUIRE(conv_variant() == 1, "conv3d_dgrad: needs the LDS-DMA conv kernels (AVT_CONV_VARIANT=1)");
  GemmNTParams p{};
  p.act = (const bf16_t*)dy;
  p.wmat = (const bf16_t*)wt;
  p.out = (bf16_t*)dx;
  p.add = (const bf16_t*)add;
  p.IT = To; p.IH = P; p.IW = Q; p.IC = K;
  p.OT = T; p.OH = H; p.OW = W;
  p.M = N * T * H * W;
  p.Ng = C;
  p.Kg = KT * R * S * K;
  p.KT = KT; p.R = R; p.S = S; p.stride = stride; p.pad = pad; p.pad_t = pad_t;
  AVT_REQUIRE((size_t)p.M * C * 2 < (1ull << 31) && (size_t)N * To * P * Q * K * 2 < (1ull << 31),
              "conv3d_dgrad: activation tensors must stay below 2 GiB (32-bit buffer offsets)");
  hipStream_t st = (hipStream_t)stream;
  for (int ph = 0; ph < 2; ++ph)
    for (int pw = 0; pw < 2; ++pw) {
      if (C % 128 == 0)
        launch_dgrad3d_class<2>(p, ph, pw, st);
      else
        launch_dgrad3d_class<1>(p, ph, pw, st);
    }
  return check_launch("conv3d_dgrad");
}

// Deferred split-K reduces, batched (avt_wgrad_reduce_batch): a trunk's wgrads leave their slabs (avt_conv2d_wgrad_defer)
// and one launch sums all of them at the end of the trunk's backward segment -- blockIdx.y = the slab, a grid-stride
// loop over its float4 positions; per position the splits in order, 8 loads in flight: the order of
// wgrad_slab_reduce_native_kernel with G = 1, so the bits are the same as the per-wgrad reduce launches'.
// (The reduces are off the backward's dgrad chain; at 32 clips per GPU their ~34 separate launches cost up to 7 % of
// the step: profiles/r6_slab_skip.txt.)
constexpr int kSlabBatch = 24;
struct SlabReduceBatch {
  int n;
  avt_slab_reduce_desc e[kSlabBatch];
};

__global__ __launch_bounds__(256) void wgrad_slab_reduce_batch_kernel(SlabReduceBatch b) {
  const avt_slab_reduce_desc& E = b.e[blockIdx.y];
  const int NW = E.wm * E.wn;
  const long long per_tile = (long long)NW * E.tm * E.tn * 4 * 64;
  const long long total = (long long)E.tiles * per_tile;
  const f32x4* s4 = reinterpret_cast<const f32x4*>(E.slab);
  const int BM = E.wm * E.tm * 32, BN = E.wn * E.tn * 32;
  for (long long f = (long long)blockIdx.x * 256 + threadIdx.x; f < total; f += (long long)gridDim.x * 256) {
    f32x4 a = {0.f, 0.f, 0.f, 0.f};
    for (int s0 = 0; s0 < E.splits; s0 += 8) {
      f32x4 v[8];
#pragma unroll
      for (int i = 0; i < 8; ++i) v[i] = s0 + i < E.splits ? s4[f + (s0 + i) * total] : f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int i = 0; i < 8; ++i) a += v[i];
    }
    const int lane = (int)(f & 63);
    long long r = f >> 6;
    const int q = (int)(r & 3);
    r >>= 2;
    const int jj = (int)(r % E.tn);
    r /= E.tn;
    const int i = (int)(r % E.tm);
    r /= E.tm;
    const int wid = (int)(r % NW);
    const int tile = (int)(r / NW);
    const int mt = tile / E.nnt, nt = tile - mt * E.nnt;
    const int wm = wid / E.wn, wn = wid % E.wn;
    const int col = nt * BN + wn * (BN / E.wn) + jj * 32 + (lane & 31);
    const int r0 = mt * BM + wm * (BM / E.wm) + i * 32 + 8 * q + 4 * (lane >> 5);
    if (col < E.ldw) {
#pragma unroll
      for (int e = 0; e < 4; ++e)
        if (r0 + e < E.Mg) E.dw[(size_t)(r0 + e) * E.ldw + col] += a[e];
    }
  }
}

// ---- per-pixel gather table of the tap-gather wgrad (conv_tn_pipe.h TAB) ----
// One entry per output pixel, padded to a whole 32-pixel k-tile with always-invalid entries: {the byte offset of input
// pixel (n, oh*stride - pad, ow*stride - pad) in the [N][H][W][Cp] bf16 tensor (32-bit, may wrap below zero: only valid
// taps are dereferenced), a mask whose bit r*S + s says that tap (r, s) lands inside the image}.  Geometry only.
__global__ __launch_bounds__(256) void wgrad_pixtab_kernel(uint2* __restrict__ tab, int npix, int npad, int P, int Q,
                                                           int H, int W, int Cp, int R, int S, int stride, int pad) {
  const int pix = blockIdx.x * 256 + threadIdx.x;
  if (pix >= npad) return;
  uint2 e = make_uint2(0u, 0u);
  if (pix < npix) {
    const int n = pix / (P * Q), rem = pix - n * (P * Q);
    const int oh = rem / Q, ow = rem - oh * Q;
    const int y0 = oh * stride - pad, x0 = ow * stride - pad;
    e.x = (((unsigned)n * (unsigned)H + (unsigned)y0) * (unsigned)W + (unsigned)x0) * (unsigned)(Cp * 2);
    for (int r = 0; r < R; ++r)
      for (int s = 0; s < S; ++s)
        if ((unsigned)(y0 + r) < (unsigned)H && (unsigned)(x0 + s) < (unsigned)W) e.y |= 1u << (r * S + s);
  }
  tab[pix] = e;
}

// A/B knob: AVT_WGRAD_PIXTAB / avt_set_wgrad_pixtab (1 default: a registered table is used; 0: the in-loop arithmetic).
// Bitwise-equal results either way.
static int g_wgrad_pixtab = -1;
static int wgrad_pixtab_enabled() {
  if (g_wgrad_pixtab < 0) g_wgrad_pixtab = getenv("AVT_WGRAD_PIXTAB") ? atoi(getenv("AVT_WGRAD_PIXTAB")) : 1;
  return g_wgrad_pixtab;
}

// the tables the caller has built and keeps alive (avt_wgrad_pixtab_register), by device and geometry
struct PixtabEntry {
  int dev, N, H, W, Cp, R, S, stride, pad;
  const void* tab;
};
static std::mutex g_pixtab_mu;
static std::vector<PixtabEntry> g_pixtabs;

static bool pixtab_geometry_ok(int N, int H, int W, int R, int S, int stride, int pad) {
  if (N < 1 || H < 1 || W < 1 || R < 1 || S < 1 || R * S > 32 || (stride != 1 && stride != 2) || pad < 0) return false;
  if (H + 2 * pad < R || W + 2 * pad < S) return false;
  const long long npix = (long long)N * conv_out(H, R, stride, pad) * conv_out(W, S, stride, pad);
  return npix >= 1 && (npix + 31) / 32 * 256 < (1ll << 31);
}

static const void* pixtab_lookup(int N, int H, int W, int Cp, int R, int S, int stride, int pad) {
  if (!wgrad_pixtab_enabled()) return nullptr;
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) return nullptr;
  std::lock_guard<std::mutex> lk(g_pixtab_mu);
  for (const PixtabEntry& e : g_pixtabs)
    if (e.dev == dev && e.N == N && e.H == H && e.W == W && e.Cp == Cp && e.R == R && e.S == S && e.stride == stride &&
        e.pad == pad)
      return e.tab;
  return nullptr;
}

// ---- the 2-D weight gradient: plan_wgrad decides everything from the shape, the knobs and what the caller brought;
// launch_wgrad names every instantiation once; avt_conv_wgrad_plan reports the plan without a GPU ----
static int g_wgrad_halo_rw = -1;  // rows per wave of the K = 64 halo wgrad: 32 (default) or 64; -1: env AVT_WGRAD_HALO_RW
static int g_row3_min_kt = -1;    // ROW3 split floor (k-tiles per split); -1: env AVT_ROW3_MIN_KT (default 8)
static int g_row3_kg = -1;        // ROW3 k groups per block (1, 2 or 4); -1: env AVT_ROW3_KG (default 2)
static int g_row3_pf = -1;  // ROW3 (KG 2): next tile's first fragments read behind the MFMAs (default: +3-4 %); -1: env AVT_ROW3_PF
// A/B knob: the fused slab reduce (conv_tn_pipe.h FUSED) for the tap-gather wgrads, avt_set_wgrad_fused / env
// AVT_WGRAD_FUSED (0 default = the separate reduce launch; 1 = fused up to g_wgrad_fused_max_bytes of other splits'
// partials per tile).  Bitwise equal where the separate reduce runs one wave per position, but SLOWER: the wgrad
// family 355 -> 214 TF/s, the step -7 % at B=32 and -1.7 % at B=128 (profiles/r6_ab_wgrad_fused.txt) -- the
// write-through partials and the last block's serial read of the other splits cost more than the reduce launch
static int g_wgrad_fused = -1;
static long long g_wgrad_fused_max_bytes = -1;

// Every knob the wgrad plan reads, resolved in this one place at the top of plan_wgrad: a setter's value, else the
// environment's (read at first use, and again after a setter's -1), else the default.
struct WgKnobs {
  int variant;  // conv_variant(): 1 = the LDS-DMA kernels
  int stem, halo, halo_rw, halo_share, row3_wm, row3_min_kt, row3_kg, row3_pf;
  int blocks, min_kt, min_kt_1x1, slab_max, wave_cost, big, nst, nst_big, slots_pct, kg, fused;
  long long fused_max_bytes;
};
static WgKnobs wgrad_knobs() {
  const auto env = [](const char* name, long long dflt) { return getenv(name) ? atoll(getenv(name)) : dflt; };
  const auto lazy = [&env](int& g, const char* name, int dflt) { return g < 0 ? (g = (int)env(name, dflt)) : g; };
  // read once per process: AVT_WGRAD_SLAB_MAX / _WAVE_COST (as avt_set_wgrad_slab_max) and the knobs without a setter
  struct Once { int min_kt_1x1, kg, halo_share, row3_wm; };
  static const Once once = [&env] {
    g_wgrad_slab_max = (int)env("AVT_WGRAD_SLAB_MAX", g_wgrad_slab_max);
    g_wgrad_wave_cost = (int)env("AVT_WGRAD_WAVE_COST", g_wgrad_wave_cost);
    return Once{(int)env("AVT_WGRAD_MIN_KT_1X1", 24), (int)env("AVT_WGRAD_KG", 2),
                (int)env("AVT_WGRAD_HALO_SHARE", 100), (int)env("AVT_ROW3_WM", 0)};
  }();
  WgKnobs k;
  k.variant = conv_variant();
  k.stem = lazy(g_stem_wgrad, "AVT_STEM_WGRAD", 1);
  k.halo = lazy(g_wgrad_halo, "AVT_WGRAD_HALO", 3);
  k.halo_rw = lazy(g_wgrad_halo_rw, "AVT_WGRAD_HALO_RW", 32);
  k.halo_share = once.halo_share; k.row3_wm = once.row3_wm;  // (row3_wm 1, A/B: 64-row ROW3 blocks at K >= 128)
  if (lazy(g_row3_min_kt, "AVT_ROW3_MIN_KT", 8) < 1) g_row3_min_kt = 1;
  k.row3_min_kt = g_row3_min_kt;
  lazy(g_row3_kg, "AVT_ROW3_KG", 2);
  k.row3_kg = (g_row3_kg == 2 || g_row3_kg == 4) ? g_row3_kg : 1;
  k.row3_pf = lazy(g_row3_pf, "AVT_ROW3_PF", 1);
  k.blocks = g_wgrad_blocks; k.min_kt = g_wgrad_min_kt; k.min_kt_1x1 = once.min_kt_1x1;
  k.slab_max = g_wgrad_slab_max; k.wave_cost = g_wgrad_wave_cost; k.kg = once.kg;
  k.big = lazy(g_wgrad_big, "AVT_WGRAD_BIG", 1);
  k.nst = lazy(g_wgrad_nst, "AVT_WGRAD_NST", 4);
  k.nst_big = lazy(g_wgrad_nst_big, "AVT_WGRAD_NST_BIG", 3);
  k.slots_pct = lazy(g_wgrad_slots_pct, "AVT_WGRAD_SLOTS_PCT", 0);
  k.fused = lazy(g_wgrad_fused, "AVT_WGRAD_FUSED", 0);
  if (g_wgrad_fused_max_bytes < 0) g_wgrad_fused_max_bytes = 1024LL * env("AVT_WGRAD_FUSED_MAX_KB", 2048);
  k.fused_max_bytes = g_wgrad_fused_max_bytes;
  return k;
}

// avt_conv_wgrad_plan's family and partials values (include/avt_tuning.h)
enum { WG_STEM = 0, WG_HALO9 = 1, WG_ROW3 = 2, WG_GATHER = 3, WG_REG = 4 };
enum { WG_SLAB_REDUCE = 0, WG_SLAB_FUSED = 1, WG_SLAB_DEFER = 2, WG_ATOMICS = 3 };

struct WgShape { int N, H, W, Cp, Creal, K, R, S, stride, pad; };
struct WgWs { size_t bytes; int tickets; bool defer; };  // what the caller brought (0 bytes, 0 tickets: none)
// Plain data, no caller pointer: the pointer members of the three geometry blocks stay null, launch_wgrad fills copies.
struct WgPlan {
  int family;          // WG_STEM .. WG_REG
  int wm, wn, tm, tn;  // waves per block and 32 x 32 tiles per wave (halo: tn = tap subtiles per wave; stem: wm = waves)
  int rw, prmax;       // halo forms: output channels per wave, LDS patch rows
  int nst;             // LDS ring stages of the instantiation launched
  int kg, pf;          // k groups per block; ROW3 (KG 2) prefetch form
  int tab;             // tap gather: the instantiation has a pixel-table form and the geometry a table layout
  int splits, kt_per_split, tiles;  // grid = tiles x splits (stem: splits = blocks, each a partial; tiles = wave tiles)
  int partials;        // WG_SLAB_REDUCE .. WG_ATOMICS
  size_t slab_bytes;   // of the workspace, 0 without a slab
  int tickets;         // of the caller's, WG_SLAB_FUSED only
  int G, red_grid, red_block;  // the separate reduce: waves per 64 slab positions (native), grid and block (halo: of
  int groups, per_group;       // the last pass, over `groups` heads of per_group splits each)
  GemmTNParams g; WgradHaloArgs ha; StemWgradArgs sa;  // the family's geometry block: gather / register-staged, halo, stem
};

// Arm 1, the 7x7/s2 stems on conv_stem_wgrad_kernel: one block per CU at most, every block's partial in its own slab
// entry -- so only with the workspace.  False: not such a stem, or no room (arm 3 takes it, register-staged, atomics).
static bool plan_wgrad_stem(WgPlan& pl, const WgShape& s, const WgKnobs& k, const WgWs& ws) {
  if (!((s.Cp == 4 || s.Cp == 1) && k.stem && s.K == 64 && s.R == 7 && s.S == 7 && s.stride == 2 && s.pad == 3 &&
        s.Creal >= 1 && s.Creal <= s.Cp && s.N >= 1))
    return false;
  const int OH = conv_out(s.H, 7, 2, 3), OW = conv_out(s.W, 7, 2, 3);
  const size_t x_bytes = (size_t)s.N * s.H * s.W * s.Cp * 2, dy_bytes = (size_t)s.N * OH * OW * 64 * 2;
  if (OH < 1 || OW < 1 || x_bytes >= (1ull << 31) || dy_bytes >= (1ull << 31)) return false;  // (32-bit offsets)
  const int nw = s.Cp == 4 ? StemWgradCfg<4>::NW : StemWgradCfg<1>::NW;
  const int tiles_per_row = (OW + 31) / 32, total_tiles = s.N * OH * tiles_per_row;
  const int grid = min((total_tiles + nw - 1) / nw, num_cus());
  const size_t slab_bytes = (size_t)grid * 64 * 49 * s.Creal * sizeof(float);
  if (ws.bytes < slab_bytes) return false;
  StemWgradArgs& a = pl.sa;
  a.x_bytes = (unsigned)x_bytes; a.dy_bytes = (unsigned)dy_bytes;
  a.N = s.N; a.IH = s.H; a.IW = s.W; a.OH = OH; a.OW = OW; a.Creal = s.Creal;
  a.tiles_per_row = tiles_per_row; a.total_tiles = total_tiles;
  pl.family = WG_STEM; pl.wm = nw; pl.wn = 1; pl.nst = 2; pl.kg = 1;
  pl.splits = grid; pl.tiles = total_tiles; pl.partials = WG_SLAB_REDUCE; pl.slab_bytes = slab_bytes;
  pl.red_grid = (64 * 49 * s.Creal + 63) / 64; pl.red_block = 1024;
  return true;
}

static constexpr int kRow3PrMax = 40;  // strip rows staged by the ROW3 form
// default form 3 takes ROW3 from this many output pixels up (B = 128: 401 k vision / 624 k audio); below
// it the fixed cost of the split partials (slab + ordered reduce) loses to the tap-gather kernel (B = 32:
// 100 k / 156 k pixels, -1.5 % per step in a same-box A/B)
static constexpr long long kRow3MinPixels = 200000;

// Arm 2, the 3x3/s1 convs on conv_wgrad_halo_kernel (conv_wgrad_halo.h): all nine taps per block (WG_HALO9), or one
// filter row (3 taps) per block (WG_ROW3: WM x 2 waves of 64 x 96 per k group, a strip of PR - 2 PW patch rows).
// False: the knob or the shape keeps the conv on arm 3.
static bool plan_wgrad_halo(WgPlan& pl, const WgShape& s, const WgKnobs& k, const WgWs& ws) {
  const int N = s.N, H = s.H, W = s.W, Cp = s.Cp, K = s.K;
  int mode = k.halo;
  if (mode == 3) mode = (K == 64 && (long long)N * H * W >= kRow3MinPixels) ? 2 : 0;
  if (!mode || s.R != 3 || s.S != 3 || s.stride != 1 || s.pad != 1 || Cp != s.Creal || Cp % 64 != 0 || K % 64 != 0 ||
      k.variant != 1)
    return false;
  WgradHaloArgs a{};
  a.N = N; a.H = H; a.W = W; a.C = Cp; a.K = K;
  const bool row3 = mode == 2;
  int WM = (K % 128 == 0) ? 2 : 1;  // 2: BM 128 (4 waves), 1: BM 64 (2 waves)
  int RW = 64;                      // output channels per wave
  if (!row3 && K == 64 && k.halo_rw == 32) {  // 4 waves of 32 x 288 (144 accumulator registers: two waves per SIMD)
    WM = 2;
    RW = 32;
  }
  if (row3 && k.row3_wm == 1) WM = 1;
  const int BM = WM * RW;  // after every WM override: the plan and the launch use the same block rows
  const int ncols = row3 ? 192 : 576;  // GEMM columns per block
  const int PRMAX = row3 ? kRow3PrMax : (WM == 2 && RW == 64) ? 160 : 72;
  // ROW3: KG groups of WM x 2 waves on interleaved k-tiles, one partial per block (WM 2: at most 2)
  const int kg = !row3 ? 1 : WM == 1 ? k.row3_kg : (k.row3_kg >= 2 ? 2 : 1);
  const int per_cu = row3 ? (WM == 1 ? 4 : 2) / kg : (WM == 2 && RW == 64) ? 1 : 2;  // resident blocks per CU
  auto staged = [&](int pr, int pw) { return row3 ? pr - 2 * pw : pr; };
  const double t_mfma = 2.0 * 32 * BM * ncols / (4 * 1024.0);
  auto cost = [&](long long tiles, int pr) {  // pr: staged patch rows
    const double fill = (32.0 * BM * 2 + pr * 128.0) / (29.0 / per_cu);
    return (double)tiles * (t_mfma > fill ? t_mfma : fill);
  };
  double best = -1;
  // raster: 32 consecutive pixels span at most ceil(31/W)+1 rows
  {
    const int span = (W >= 32 ? 2 : (31 + W - 1) / W + 1);
    const int pr = (span + 2) * (W + 2);
    if (!row3 && staged(pr, W + 2) <= PRMAX) {  // (ROW3: windows only -- fixed fragment rows)
      const long long tiles = (long long)(H * W + 31) / 32;
      best = cost(tiles, staged(pr, W + 2));
      a.raster = 1; a.R = 1; a.CW = 32; a.lcw = 5; a.wcols = 1; a.tiles_img = (int)tiles; a.PW = W + 2; a.PR = pr;
    }
  }
  const int shapes[4][2] = {{1, 32}, {2, 16}, {4, 8}, {8, 4}};
  for (auto& sh : shapes) {
    const int r = sh[0], cw = sh[1];
    const int pr = (r + 2) * (cw + 2);
    if (staged(pr, cw + 2) > PRMAX) continue;
    const int bands = (H + r - 1) / r, wcols = (W + cw - 1) / cw;
    const double c = cost((long long)bands * wcols, staged(pr, cw + 2));
    if (best < 0 || c < best * 0.999) {
      best = c;
      a.raster = 0; a.R = r; a.CW = cw; a.lcw = 31 - __builtin_clz(cw); a.wcols = wcols; a.tiles_img = bands * wcols;
      a.PW = cw + 2; a.PR = pr;
    }
  }
  if (best < 0) return false;
  a.nkt = N * a.tiles_img;
  const int per_split = (K / BM) * (Cp / 64) * (row3 ? 3 : 1);
  // (A/B, env AVT_WGRAD_HALO_SHARE, default 100: the share of the chip's block slots the split count assumes)
  const long long slots = max(1LL, (long long)num_cus() * per_cu * min(max(k.halo_share, 1), 100) / 100);
  int splits = (int)(slots / per_split);
  if (row3) {  // at least row3_min_kt k-tiles per split: the slab (splits x 147 KB at K 64) is the cost at small N
    const int cap = a.nkt / k.row3_min_kt;
    if (splits > cap) splits = cap;
  }
  if (splits < 1) splits = 1;
  if (splits > a.nkt) splits = a.nkt;
  const int kps = (a.nkt + splits - 1) / splits;
  a.kt_per_split = kps;
  a.splits = (a.nkt + kps - 1) / kps;  // every split non-empty
  a.div_w = make_magic((unsigned)W);
  a.div_tiles = make_magic((unsigned)a.tiles_img);
  a.div_wcols = make_magic((unsigned)a.wcols);
  a.dy_bytes = (unsigned)((size_t)N * H * W * K * 2);
  a.x_bytes = (unsigned)((size_t)N * H * W * Cp * 2);
  pl.ha = a;
  pl.family = row3 ? WG_ROW3 : WG_HALO9;
  pl.wm = WM; pl.wn = 2; pl.tm = RW / 32; pl.tn = row3 ? 3 : 9;
  pl.rw = RW; pl.prmax = PRMAX; pl.nst = row3 ? 4 : (WM == 2 && RW == 64) ? 5 : 6;
  pl.kg = kg; pl.pf = row3 && WM == 1 && kg == 2 && k.row3_pf;
  pl.splits = a.splits; pl.kt_per_split = kps; pl.tiles = per_split;
  // without the workspace the split partials are added with fp32 atomics
  const size_t want = a.splits > 1 ? (size_t)a.splits * K * 9 * Cp * sizeof(float) : 0;
  pl.slab_bytes = ws.bytes >= want ? want : 0;
  pl.partials = pl.slab_bytes > 0 ? WG_SLAB_REDUCE : WG_ATOMICS;
  if (pl.slab_bytes > 0) {  // ordered: groups of per_group splits, then the group heads
    pl.per_group = 16; pl.groups = (a.splits + pl.per_group - 1) / pl.per_group;
    // the final pass is latency-bound (one thread per 4 outputs, a serial chain of entries): 64-thread blocks
    pl.red_grid = (int)(((long long)K * 9 * Cp / 4 + 63) / 64); pl.red_block = 64;
  }
  return true;
}

// Arm 3, every other conv: the tap-gather kernel (conv_tn_pipe_kernel, C % 8 == 0), or the register-staged
// gemm_tn_kernel (the stems without their workspace, and everything under avt_set_conv_variant(0)).
static void plan_wgrad_gemm(WgPlan& pl, const WgShape& s, const WgKnobs& k, const WgWs& ws) {
  const int N = s.N, Cp = s.Cp, K = s.K, R = s.R, S = s.S;
  GemmTNParams& p = pl.g;
  p.Mg = K; p.H = s.H; p.W = s.W; p.Cp = Cp; p.Creal = s.Creal;
  p.P = conv_out(s.H, R, s.stride, s.pad);
  p.Q = conv_out(s.W, S, s.stride, s.pad);
  p.R = R; p.S = S; p.stride = s.stride; p.pad = s.pad;
  p.Kred = N * p.P * p.Q;
  const int ncols = R * S * Cp;
  const bool pipe = (Cp % 8 == 0) && k.variant == 1;
  int BN = (ncols % 128 == 0 || ncols > 128) ? 128 : 64;
  int BM = (K % 128 == 0 && Cp % 8 == 0) || (K % 128 == 0 && Cp == 4) ? 128 : 64;
  // 8-wave 256-wide tiles halve the LDS fill bytes per flop where the GEMM is wide enough
  // (layer4: K_out 512, R*S*C >= 2304); split-K supplies the parallelism
  if (pipe && k.big) {
    if (K % 256 == 0 && K >= 512 && BN == 128) BM = 256;  // measured: a loss on layer3 (K_out 256)
    if (ncols >= 2048 && BM == 256) BN = 256;
  }
  p.Ng = ((ncols + BN - 1) / BN) * BN;
  pl.tiles = (p.Mg / BM) * (p.Ng / BN);
  const int nkt = (p.Kred + 31) / 32;
  // Split-K count.  The grid runs in "waves" of resident blocks (CUs x blocks per CU, set by the
  // ring's LDS: 4 stages x 32 pixels x (BM+BN) bf16 for the 4-wave tiles, 3 stages for the 8-wave
  // ones, whose 256x256 form is also held to one block per CU by its registers).  For w = 1..4
  // waves take the largest split count that fits, s_w = floor(w*slots/tiles), and keep the one
  // with the least w * (ceil(nkt/s_w) + wave_cost) -- k-tiles per block plus its fixed
  // prologue/epilogue cost.
  // 1x1 convs (the downsample shortcuts): a k-tile is only 32 pixels x (BM + BN) operand rows while
  // the epilogue still writes a BM x BN fp32 tile, so blocks need deeper K ranges than the wave
  // model picks (measured, tools/conv_bench.py: min 24 k-tiles takes the six downsample wgrads from
  // 0.239 to 0.143 ms at B = 128; the 3x3 shapes keep their optimum at 4; env AVT_WGRAD_MIN_KT_1X1)
  const int min_kt = (R * S == 1) ? max(k.min_kt, k.min_kt_1x1) : k.min_kt;
  const bool big = BM == 256 || BN == 256, big2 = BM == 256 && BN == 256;
  // ring depth: 4 stages (4-wave tiles: two blocks per CU at 128 x 128) / 3 (8-wave); a deeper ring
  // (AVT_WGRAD_NST / AVT_WGRAD_NST_BIG, or avt_set_wgrad_nst) keeps more k-tiles in flight for a
  // block alone on its CU -- the small-batch regime, where a block's k range is short and its DMA
  // latency is exposed (one stage = 32 pixels x (BM + BN) bf16).  The 256 x 128 8-wave tile always
  // runs the 3-stage ring: nst_big is the 256 x 256 tile's.  nst_knob, the knob's value, feeds the occupancy model and
  // the kg rule; pl.nst is the ring of the instantiation launched, the nearest at or below it: they differ for knob
  // values 5 and 7 (launched 4 and 6) and for whatever an environment variable sets outside the setter's range.
  const int nst_knob = big2 ? k.nst_big : big ? 3 : k.nst;
  int splits;
  if (k.blocks > 0) {
    splits = k.blocks / pl.tiles;
  } else {
    int occ = max(1, 163840 / (nst_knob * 64 * (BM + BN)));
    if (big2) occ = 1;
    // The share of the chip's block slots the model assumes the wgrad has: with both trunks' backward on two streams a
    // wgrad shares the chip with the other trunk's kernels, and fewer splits mean fewer partials through the slab and
    // a shorter reduce.  Auto (default): 65 % for a batch of <= 32, 75 % for <= 64, else 100 % -- measured same-box
    // (profiles/r6_ab_wgrad_slots*.txt): 65 % is +3.3 % at B=32, 75 % +0.7 % at B=64, and 50 % -1.8 % at B=128.
    // AVT_WGRAD_SLOTS_PCT / avt_set_wgrad_slots_pct fix it (1-100; 0 = auto).
    const int slots_pct = k.slots_pct > 0 ? min(k.slots_pct, 100) : N <= 32 ? 65 : N <= 64 ? 75 : 100;
    const long long slots = max(1LL, (long long)num_cus() * occ * slots_pct / 100);
    long long best = -1;
    splits = 1;
    for (int w = 1; w <= 4; ++w) {
      const int s_w = (int)(w * slots / pl.tiles);
      if (s_w < 1) continue;
      const int kps_w = max(min_kt, (nkt + s_w - 1) / s_w);
      const long long waves = (((long long)pl.tiles * ((nkt + kps_w - 1) / kps_w)) + slots - 1) / slots;
      const long long cost = waves * (kps_w + k.wave_cost);
      if (best < 0 || cost < best) {
        best = cost;
        splits = s_w;
      }
    }
  }
  if (splits < 1) splits = 1;
  int kps = (nkt + splits - 1) / splits;
  if (kps < min_kt) kps = min_kt;
  pl.splits = (nkt + kps - 1) / kps;
  // two wave groups per block (AVT_WGRAD_KG, default 2): the pairs of blocks the plan puts on one CU
  // become one 8-wave block over both k ranges with ONE partial tile -- half the split-K slab bytes
  // (or atomics) at the same waves per CU; 4-wave tiles on the 4-stage ring (2 x 64 KB of LDS at 128 x 128)
  pl.kg = 1;
  const int pair_occ = 163840 / (nst_knob * 64 * (BM + BN));  // 4-wave blocks per CU (2 at 128 x 128)
  // (3x3 only: the 1x1 shortcuts' deep k ranges lost 25-30 % at B = 128 as pairs)
  if (k.kg >= 2 && pipe && !big && nst_knob == 4 && pair_occ == 2 && pl.splits >= 2 && R * S > 1) {
    pl.kg = 2;
    kps *= 2;
    pl.splits = (nkt + kps - 1) / kps;
  }
  p.kt_per_split = pl.kt_per_split = kps;
  pl.family = pipe ? WG_GATHER : WG_REG;
  pl.wm = BM == 256 ? 4 : 2; pl.wn = 2; pl.tm = BM == 64 ? 1 : 2; pl.tn = BN / 64;
  pl.nst = !pipe ? 2 : big2 ? (nst_knob >= 5 ? 5 : nst_knob == 4 ? 4 : 3) : big ? 3
           : pl.kg == 2 ? 4 : nst_knob >= 8 ? 8 : nst_knob >= 6 ? 6 : 4;
  // the base ring's instantiations have the fused-reduce (FUSED) and pixel-table (TAB) forms; the deeper-ring A/B
  // variants keep the separate reduce and the in-loop arithmetic
  const bool base_ring = pipe && pl.nst == (big ? 3 : 4);
  pl.tab = base_ring && pixtab_geometry_ok(N, s.H, s.W, R, S, s.stride, s.pad);
  // slab + reduce pass for moderate split counts (measured faster on layer3/4); very deep splits
  // (layer1/2: 100-200 splits of a small output) keep the fp32 atomics, which overlap the compute
  // (the slab holds whole tiles in register order: splits x Mg x Ng, conv_tn_pipe.h)
  const size_t want = (pipe && pl.splits > 1 && pl.splits <= k.slab_max) ? (size_t)pl.splits * p.Mg * p.Ng * sizeof(float) : 0;
  pl.slab_bytes = ws.bytes >= want ? want : 0; pl.partials = WG_ATOMICS;
  if (pl.slab_bytes == 0) return;
  if (base_ring && k.fused && ws.tickets >= pl.tiles && (long long)(pl.splits - 1) * BM * BN * 4 <= k.fused_max_bytes) {
    pl.partials = WG_SLAB_FUSED;  // the last block of each tile sums the tile's partials
    pl.tickets = pl.tiles;
    return;
  }
  // G waves per 64 slab positions: 1 where the positions alone give ~64 K threads, else up to min(splits, 16)
  const long long positions = (long long)pl.tiles * pl.wm * pl.wn * pl.tm * pl.tn * 4 * 64;
  pl.G = 1;
  while (pl.G * 2 <= pl.splits && pl.G * 2 <= 16 && positions * pl.G < 65536) pl.G *= 2;
  pl.partials = (ws.defer && pl.G == 1) ? WG_SLAB_DEFER : WG_SLAB_REDUCE;  // deferred: the batched reduce's order is G = 1's
  if (pl.partials == WG_SLAB_DEFER) return;
  const int nwb = pl.G > 4 ? pl.G : 4, ngrp = nwb / pl.G;
  pl.red_grid = (int)max(1LL, min(4096LL, (positions + 64LL * ngrp - 1) / (64LL * ngrp)));
  pl.red_block = nwb * 64;
}

static WgPlan plan_wgrad(const WgShape& s, const WgWs& ws) {
  const WgKnobs k = wgrad_knobs();
  WgPlan pl{};
  if (!plan_wgrad_stem(pl, s, k, ws) && !plan_wgrad_halo(pl, s, k, ws)) plan_wgrad_gemm(pl, s, k, ws);
  return pl;
}

// Launches a plan.  Every wgrad kernel and reduce instantiation is named here, once.  dry: the same table walk, nothing
// launched (avt_conv_wgrad_plan).  False: no such instantiation.
static bool launch_wgrad(const WgPlan& pl, const bf16_t* x, const bf16_t* dy, float* dw, void* workspace, int* tickets,
                         avt_slab_reduce_desc* defer, hipStream_t st, bool dry = false) {
  float* slab = pl.slab_bytes > 0 ? (float*)workspace : nullptr;
  const dim3 grid(pl.tiles * pl.splits);
  const auto tile = [&pl](int wm, int wn, int tm, int tn) { return pl.wm == wm && pl.wn == wn && pl.tm == tm && pl.tn == tn; };
  bool found = false;
#define AVT_LAUNCH(KERNEL, GRID, BLOCK, LDS, ...)                                 \
  {                                                                               \
    if (!dry) hipLaunchKernelGGL(KERNEL, GRID, dim3(BLOCK), LDS, st, __VA_ARGS__); \
    found = true;                                                                 \
  }
  switch (pl.family) {
    case WG_STEM: {
      StemWgradArgs a = pl.sa;
      a.x = x; a.dy = dy; a.slab = slab;
#define AVT_WSTEM(C) \
  if (pl.wm == StemWgradCfg<C>::NW) AVT_LAUNCH(conv_stem_wgrad_kernel<C>, dim3(pl.splits), pl.wm * 64, stem_wgrad_lds_bytes<C>(), a)
      AVT_WSTEM(4)
      AVT_WSTEM(1)
#undef AVT_WSTEM
      if (found)
        AVT_LAUNCH(stem_wgrad_reduce_kernel, dim3(pl.red_grid), pl.red_block, 0, (const float*)slab, pl.splits,
                   64 * 49 * a.Creal, dw)
      return found;
    }
    case WG_HALO9:
    case WG_ROW3: {
      WgradHaloArgs a = pl.ha;
      a.x = x; a.dy = dy; a.dw = dw; a.slab = slab;
#define AVT_WHALO(WM, NST, PRMAX, RW, ROW3, KG, PF)                                                               \
  if (pl.wm == WM && pl.nst == NST && pl.prmax == PRMAX && pl.rw == RW && (pl.family == WG_ROW3) == ROW3 &&      \
      pl.kg == KG && (pl.pf != 0) == PF)                                                                          \
    AVT_LAUNCH((conv_wgrad_halo_kernel<WM, NST, PRMAX, RW, ROW3, KG, PF>), grid, WM * 2 * KG * 64, 0, a)
      AVT_WHALO(2, 4, kRow3PrMax, 64, true, 2, false)
      AVT_WHALO(2, 4, kRow3PrMax, 64, true, 1, false)
      AVT_WHALO(1, 4, kRow3PrMax, 64, true, 4, false)
      AVT_WHALO(1, 4, kRow3PrMax, 64, true, 2, true)
      AVT_WHALO(1, 4, kRow3PrMax, 64, true, 2, false)
      AVT_WHALO(1, 4, kRow3PrMax, 64, true, 1, false)
      AVT_WHALO(2, 6, 72, 32, false, 1, false)   // K = 64: 4 waves of 32 x 288
      AVT_WHALO(2, 5, 160, 64, false, 1, false)
      AVT_WHALO(1, 6, 72, 64, false, 1, false)
#undef AVT_WHALO
      if (found && slab != nullptr) {  // ordered: groups of per_group splits, then the group heads
        const long long n = (long long)a.K * 9 * a.C;
        const bool two = pl.groups > 1;
        if (two)
          AVT_LAUNCH(wgrad_halo_reduce_kernel, dim3((unsigned)((n / 4 + 255) / 256), (unsigned)pl.groups), 256, 0, slab,
                     a.splits, 1, pl.per_group, n, dw)
        AVT_LAUNCH(wgrad_halo_reduce_kernel, dim3(pl.red_grid, 1), pl.red_block, 0, slab, two ? pl.groups : a.splits,
                   two ? pl.per_group : 1, two ? pl.groups : a.splits, n, dw)
      }
      return found;
    }
    case WG_REG: {
      GemmTNParams p = pl.g;
      p.x = x; p.dy = dy; p.dw = dw;
      const int cvec = p.Cp % 8 == 0 ? 8 : p.Cp;
#define AVT_TNREG(CVEC, BM, BN) \
  if (cvec == CVEC && tile(2, 2, BM / 64, BN / 64)) AVT_LAUNCH((gemm_tn_kernel<CVEC, BM, BN>), dim3(pl.tiles, pl.splits), 256, 0, p)
      AVT_TNREG(4, 128, 128)
      AVT_TNREG(4, 64, 128)
      AVT_TNREG(1, 64, 128)
      AVT_TNREG(1, 64, 64)
      AVT_TNREG(8, 128, 128)
      AVT_TNREG(8, 64, 128)
      AVT_TNREG(8, 128, 64)
      AVT_TNREG(8, 64, 64)
#undef AVT_TNREG
      return found;
    }
    case WG_GATHER: {
      GemmTNPipeParams pp;
      GemmTNParams& p = pp.p = pl.g;
      p.x = x; p.dy = dy; p.dw = dw;
      pp.div_pq = make_magic((unsigned)(p.P * p.Q));
      pp.div_q = make_magic((unsigned)p.Q);
      pp.dy_bytes = (unsigned)((size_t)p.Kred * p.Mg * 2);
      pp.x_bytes = (unsigned)((size_t)(p.Kred / (p.P * p.Q)) * p.H * p.W * p.Cp * 2);
      pp.slab = slab; pp.slab_bytes = (unsigned)pl.slab_bytes; pp.splits = pl.splits;
      pp.cnt = pl.partials == WG_SLAB_FUSED ? tickets : nullptr;
      // the registered per-pixel table of this geometry: per device and stateful, so looked up here
      pp.tab = pl.tab && !dry ? pixtab_lookup(p.Kred / (p.P * p.Q), p.H, p.W, p.Cp, p.R, p.S, p.stride, p.pad) : nullptr;
      const bool fused = pl.partials == WG_SLAB_FUSED, tab = pp.tab != nullptr;
#define AVT_TN(WM, WN, TM, TN, NST, KG, FUSED, TAB)                                     \
  if (tile(WM, WN, TM, TN) && pl.nst == NST && pl.kg == KG && fused == FUSED && tab == TAB) \
    AVT_LAUNCH((conv_tn_pipe_kernel<WM, WN, TM, TN, NST, KG, FUSED, TAB>), grid, WM * WN * 64 * KG, 0, pp)
#define AVT_TN4(WM, WN, TM, TN, NST, KG) /* a base-ring tile: plain, FUSED, TAB, both */ \
  AVT_TN(WM, WN, TM, TN, NST, KG, false, false)                                          \
  AVT_TN(WM, WN, TM, TN, NST, KG, true, false)                                           \
  AVT_TN(WM, WN, TM, TN, NST, KG, false, true)                                           \
  AVT_TN(WM, WN, TM, TN, NST, KG, true, true)
#define AVT_TN_4WAVE(TM, TN) /* a 4-wave tile: the 4-stage ring alone and as a pair of k groups, the deeper rings */ \
  AVT_TN4(2, 2, TM, TN, 4, 1)                                                                                         \
  AVT_TN4(2, 2, TM, TN, 4, 2)                                                                                         \
  AVT_TN(2, 2, TM, TN, 6, 1, false, false)                                                                            \
  AVT_TN(2, 2, TM, TN, 8, 1, false, false)
      AVT_TN4(4, 2, 2, 4, 3, 1)  // 256 x 256
      AVT_TN(4, 2, 2, 4, 4, 1, false, false)
      AVT_TN(4, 2, 2, 4, 5, 1, false, false)
      AVT_TN4(4, 2, 2, 2, 3, 1)  // 256 x 128
      AVT_TN_4WAVE(2, 2)
      AVT_TN_4WAVE(1, 2)
      AVT_TN_4WAVE(2, 1)
      AVT_TN_4WAVE(1, 1)
#undef AVT_TN_4WAVE
#undef AVT_TN4
#undef AVT_TN
      if (!found || pl.partials == WG_ATOMICS || pl.partials == WG_SLAB_FUSED) return found;
      if (!dry && diag_skip(4, st)) return true;
      if (pl.partials == WG_SLAB_DEFER) {  // left for the batched reduce
        if (!dry) *defer = avt_slab_reduce_desc{slab, dw, pl.splits, pl.tiles, p.Ng / (pl.wn * pl.tn * 32), p.Mg,
                                                p.R * p.S * p.Creal, pl.wm, pl.wn, pl.tm, pl.tn};
        return true;
      }
      found = false;
#define AVT_RED(WM, WN, TM, TN)                                                                                       \
  if (tile(WM, WN, TM, TN))                                                                                           \
    AVT_LAUNCH((wgrad_slab_reduce_native_kernel<WM, WN, TM, TN>), dim3(pl.red_grid), pl.red_block, 0, slab, pl.splits, \
               pl.tiles, p.Ng / (WN * TN * 32), p.Mg, p.R * p.S * p.Creal, pl.G, dw)
      AVT_RED(4, 2, 2, 4)
      AVT_RED(4, 2, 2, 2)
      AVT_RED(2, 2, 2, 2)
      AVT_RED(2, 2, 2, 1)
      AVT_RED(2, 2, 1, 2)
      AVT_RED(2, 2, 1, 1)
#undef AVT_RED
      return found;
    }
  }
#undef AVT_LAUNCH
  return false;
}

extern "C" int avt_set_halo_tps2(int on) {
  AVT_REQUIRE(on >= -1 && on <= 1, "avt_set_halo_tps2: %d (0 one tap per barrier, 1 two, -1 env AVT_HALO_TPS2)", on);
  g_halo_tps2 = on;
  return AVT_OK;
}

extern "C" int avt_set_halo3d(int on) {
  AVT_REQUIRE(on >= -1 && on <= 2, "avt_set_halo3d: %d (0 tap gather, 1 halo for K %% 128 == 0, 2 also K = 64, -1 env "
              "AVT_HALO3D)", on);
  g_halo3d = on;
  return AVT_OK;
}

extern "C" int avt_set_wgrad_row3(int kg, int min_kt, int pf) {
  AVT_REQUIRE(kg == -1 || kg == 1 || kg == 2 || kg == 4, "avt_set_wgrad_row3: kg=%d (1, 2 or 4)", kg);
  AVT_REQUIRE(min_kt == -1 || min_kt >= 1, "avt_set_wgrad_row3: min_kt=%d", min_kt);
  AVT_REQUIRE(pf >= -1 && pf <= 1, "avt_set_wgrad_row3: pf=%d", pf);
  // -1 resets a value to its environment default (re-read on next use), as the sibling setters do
  g_row3_kg = kg;
  g_row3_min_kt = min_kt;
  g_row3_pf = pf;
  return AVT_OK;
}

extern "C" int avt_set_wgrad_pixtab(int on) {
  AVT_REQUIRE(on >= -1 && on <= 1, "avt_set_wgrad_pixtab: %d (0 in-loop arithmetic, 1 registered tables, -1 env "
              "AVT_WGRAD_PIXTAB)", on);
  g_wgrad_pixtab = on;
  return AVT_OK;
}

extern "C" size_t avt_wgrad_pixtab_bytes(int N, int H, int W, int R, int S, int stride, int pad) {
  using namespace avt;
  if (!pixtab_geometry_ok(N, H, W, R, S, stride, pad)) return 0;
  const long long npix = (long long)N * conv_out(H, R, stride, pad) * conv_out(W, S, stride, pad);
  return (size_t)((npix + 31) / 32 * 32) * 8;
}

extern "C" int avt_wgrad_pixtab_build(void* tab, int N, int H, int W, int Cp, int R, int S, int stride, int pad,
                                      void* stream) {
  using namespace avt;
  AVT_REQUIRE(tab, "wgrad_pixtab_build: null table");
  AVT_REQUIRE(Cp >= 1 && pixtab_geometry_ok(N, H, W, R, S, stride, pad),
              "wgrad_pixtab_build: no table form for this geometry (at most 32 taps, stride 1 or 2)");
  const int P = conv_out(H, R, stride, pad), Q = conv_out(W, S, stride, pad);
  const int npix = N * P * Q, npad = (npix + 31) / 32 * 32;
  hipLaunchKernelGGL(wgrad_pixtab_kernel, dim3((npad + 255) / 256), dim3(256), 0, (hipStream_t)stream, (uint2*)tab,
                     npix, npad, P, Q, H, W, Cp, R, S, stride, pad);
  return check_launch("wgrad_pixtab_build");
}

extern "C" int avt_wgrad_pixtab_register(const void* tab, int N, int H, int W, int Cp, int R, int S, int stride,
                                         int pad) {
  using namespace avt;
  AVT_REQUIRE(Cp >= 1 && pixtab_geometry_ok(N, H, W, R, S, stride, pad),
              "wgrad_pixtab_register: no table form for this geometry (at most 32 taps, stride 1 or 2)");
  int dev = 0;
  AVT_REQUIRE(hipGetDevice(&dev) == hipSuccess, "wgrad_pixtab_register: no current device");
  std::lock_guard<std::mutex> lk(g_pixtab_mu);
  for (size_t i = 0; i < g_pixtabs.size(); ++i) {
    const PixtabEntry& e = g_pixtabs[i];
    if (e.dev == dev && e.N == N && e.H == H && e.W == W && e.Cp == Cp && e.R == R && e.S == S && e.stride == stride &&
        e.pad == pad) {
      g_pixtabs.erase(g_pixtabs.begin() + (long)i);
      break;
    }
  }
  if (tab != nullptr) g_pixtabs.push_back(PixtabEntry{dev, N, H, W, Cp, R, S, stride, pad, tab});
  return AVT_OK;
}

extern "C" int avt_set_wgrad_halo(int on) {
  AVT_REQUIRE(on >= -1 && on <= 3, "avt_set_wgrad_halo: %d (0 off, 1 nine taps, 2 one filter row per block, 3 = 2 for K 64, -1 env)", on);
  avt::g_wgrad_halo = on;
  return AVT_OK;
}

extern "C" int avt_set_wgrad_fused(int on, int max_kb) {
  AVT_REQUIRE(on >= -1 && on <= 1, "avt_set_wgrad_fused: %d (0 separate reduce, 1 fused, -1 env AVT_WGRAD_FUSED)", on);
  AVT_REQUIRE(max_kb >= -1, "avt_set_wgrad_fused: max_kb=%d", max_kb);
  g_wgrad_fused = on;
  g_wgrad_fused_max_bytes = max_kb < 0 ? -1 : 1024LL * max_kb;
  return AVT_OK;
}

// what every wgrad entry point and avt_conv_wgrad_plan refuse
static int wgrad_check_shape(const WgShape& s) {
  AVT_REQUIRE(s.K % 64 == 0, "conv2d_wgrad: K=%d must be a multiple of 64", s.K);
  AVT_REQUIRE(s.Cp % 8 == 0 || s.Cp == 4 || s.Cp == 1, "conv2d_wgrad: C=%d unsupported", s.Cp);
  AVT_REQUIRE(s.Creal <= s.Cp, "conv2d_wgrad: Creal > Cp");
  AVT_REQUIRE(s.Cp % 8 != 0 || s.Creal == s.Cp, "conv2d_wgrad: channel padding only for the stems");
  AVT_REQUIRE(s.N >= 1 && s.H >= 1 && s.W >= 1 && s.Creal >= 1 && s.K >= 64 && s.R >= 1 && s.S >= 1 && s.pad >= 0 &&
                  (s.stride == 1 || s.stride == 2) && s.H + 2 * s.pad >= s.R && s.W + 2 * s.pad >= s.S,
              "conv2d_wgrad: empty input, taps or output, negative padding, or a stride other than 1 and 2");
  return AVT_OK;
}

// the two size queries plan for a caller who brings what they size
static const WgWs kWsAnySlab{~(size_t)0, 0, false}, kWsAnyTickets{~(size_t)0, 1 << 30, false};

// tickets the fused wgrad slab reduce needs for this conv (avt_conv2d_wgrad_tk), 0: the shape does not use it
extern "C" int avt_conv2d_wgrad_tickets(int N, int H, int W, int Cp, int Creal, int K, int R, int S, int stride,
                                        int pad) {
  return plan_wgrad(WgShape{N, H, W, Cp, Creal, K, R, S, stride, pad}, kWsAnyTickets).tickets;
}

extern "C" size_t avt_conv2d_wgrad_workspace(int N, int H, int W, int Cp, int Creal, int K, int R, int S, int stride,
                                             int pad) {
  return plan_wgrad(WgShape{N, H, W, Cp, Creal, K, R, S, stride, pad}, kWsAnySlab).slab_bytes;
}

static int conv2d_wgrad_impl(const void* x, const void* dy, float* dw, const WgShape& s, void* workspace,
                             size_t ws_bytes, int* tickets, int n_tickets, avt_slab_reduce_desc* defer, void* stream) {
  AVT_REQUIRE(x && dy && dw, "conv2d_wgrad: null pointer");
  if (const int rc = wgrad_check_shape(s)) return rc;
  const WgPlan pl = plan_wgrad(s, WgWs{workspace ? ws_bytes : 0, tickets ? n_tickets : 0, defer != nullptr});
  AVT_REQUIRE(launch_wgrad(pl, (const bf16_t*)x, (const bf16_t*)dy, dw, workspace, tickets, defer, (hipStream_t)stream),
              "conv2d_wgrad: no kernel for the plan");
  return check_launch(pl.family == WG_STEM ? "conv2d_wgrad(stem)"
                      : pl.family == WG_HALO9 || pl.family == WG_ROW3 ? "conv2d_wgrad(halo)" : "conv2d_wgrad");
}

// dw += wgrad.  With a workspace of avt_conv2d_wgrad_workspace() bytes the split-K partials go
// through an fp32 slab + one reduction pass (deterministic, 2x cheaper than atomics); without it
// (or for the stems) they are added with fp32 atomics.  dw must hold zero or a gradient to add to.
// tickets: >= avt_conv2d_wgrad_tickets() ints, zero on entry (the kernel leaves them zero), or null: the split-K slab
// is summed by the last block of each tile instead of a separate reduce launch (same bits)
extern "C" int avt_conv2d_wgrad_tk(const void* x, const void* dy, float* dw, int N, int H, int W, int Cp, int Creal,
                                   int K, int R, int S, int stride, int pad, void* workspace, size_t ws_bytes,
                                   int* tickets, int n_tickets, void* stream) {
  return conv2d_wgrad_impl(x, dy, dw, WgShape{N, H, W, Cp, Creal, K, R, S, stride, pad}, workspace, ws_bytes, tickets,
                           n_tickets, nullptr, stream);
}

extern "C" int avt_conv2d_wgrad(const void* x, const void* dy, float* dw, int N, int H, int W, int Cp, int Creal,
                                int K, int R, int S, int stride, int pad, void* workspace, size_t ws_bytes,
                                void* stream) {
  return avt_conv2d_wgrad_tk(x, dy, dw, N, H, W, Cp, Creal, K, R, S, stride, pad, workspace, ws_bytes, nullptr, 0,
                             stream);
}

extern "C" int avt_conv2d_wgrad_defer(const void* x, const void* dy, float* dw, int N, int H, int W, int Cp, int Creal,
                                      int K, int R, int S, int stride, int pad, void* workspace, size_t ws_bytes,
                                      avt_slab_reduce_desc* desc, void* stream) {
  AVT_REQUIRE(desc, "conv2d_wgrad_defer: null descriptor");
  desc->splits = 0;
  return conv2d_wgrad_impl(x, dy, dw, WgShape{N, H, W, Cp, Creal, K, R, S, stride, pad}, workspace, ws_bytes, nullptr,
                           0, desc, stream);
}

// The plan of a wgrad call, from its shape, the current knobs and what the caller brings (include/avt_tuning.h): no
// GPU, no launch.
extern "C" int avt_conv_wgrad_plan(int N, int H, int W, int Cp, int Creal, int K, int R, int S, int stride, int pad,
                                   int ws_mode, int* plan) {
  AVT_REQUIRE(plan, "conv_wgrad_plan: null pointer");
  AVT_REQUIRE(ws_mode >= 0 && ws_mode <= 3,
              "conv_wgrad_plan: ws_mode=%d (0 no workspace, 1 the workspace, 2 with tickets, 3 with a defer descriptor)", ws_mode);
  const WgShape s{N, H, W, Cp, Creal, K, R, S, stride, pad};
  if (const int rc = wgrad_check_shape(s)) return rc;  // (the geometry too: what the entry points refuse)
  WgWs ws{0, 0, ws_mode == 3};
  if (ws_mode >= 1) ws.bytes = plan_wgrad(s, kWsAnySlab).slab_bytes;
  if (ws_mode == 2) ws.tickets = plan_wgrad(s, kWsAnyTickets).tickets;
  const WgPlan pl = plan_wgrad(s, ws);
  const bool found = launch_wgrad(pl, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, true);
  const int out[AVT_WGRAD_PLAN_INTS] = {pl.family, pl.wm, pl.wn, pl.tm, pl.tn, pl.rw, pl.prmax, pl.nst, pl.kg, pl.pf,
                                        pl.tab, pl.splits, pl.kt_per_split, pl.tiles, pl.partials,
                                        (int)(pl.slab_bytes & 0x7fffffff), (int)(pl.slab_bytes >> 31), pl.tickets,
                                        pl.G, pl.red_grid, pl.red_block, pl.groups, pl.per_group, found ? 1 : 0};
  for (int i = 0; i < AVT_WGRAD_PLAN_INTS; ++i) plan[i] = out[i];
  return AVT_OK;
}

extern "C" int avt_wgrad_reduce_batch(const avt_slab_reduce_desc* descs, int n, void* stream) {
  AVT_REQUIRE(n >= 0 && (n == 0 || descs), "wgrad_reduce_batch: bad arguments");
  hipStream_t st = (hipStream_t)stream;
  for (int k0 = 0; k0 < n; k0 += kSlabBatch) {
    SlabReduceBatch b{};
    b.n = n - k0 < kSlabBatch ? n - k0 : kSlabBatch;
    long long maxpos = 0;
    for (int k = 0; k < b.n; ++k) {
      const avt_slab_reduce_desc& d = descs[k0 + k];
      AVT_REQUIRE(d.slab && d.dw && d.splits >= 1 && d.tiles >= 1 && d.nnt >= 1 && d.wm >= 1 && d.wn >= 1 &&
                      d.tm >= 1 && d.tn >= 1,
                  "wgrad_reduce_batch: descriptor %d is not from avt_conv2d_wgrad_defer", k0 + k);
      b.e[k] = d;
      const long long pos = (long long)d.tiles * d.wm * d.wn * d.tm * d.tn * 4 * 64;
      maxpos = pos > maxpos ? pos : maxpos;
    }
    long long gx = (maxpos + 255) / 256;
    if (gx > 1024) gx = 1024;
    if (b.n > 0)
      hipLaunchKernelGGL(wgrad_slab_reduce_batch_kernel, dim3((unsigned)gx, (unsigned)b.n), dim3(256), 0, st, b);
  }
  return check_launch("wgrad_reduce_batch");
}

