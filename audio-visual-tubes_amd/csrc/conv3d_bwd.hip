// Conv3d weight gradient of the R3D-18 video trunk (models/resnet3D.py:14-20 conv3x3x3, autograd's backward of
// BasicBlock.forward 45-61): temporal stride 1, spatial stride 1 or 2, NDHWC bf16 activations.
//
//   DW[k][(kt,r,s,c)] = sum over the N*T*P*Q output positions of DY[pos][k] * X(pos; kt,r,s,c)
//
// The 2-D TN pipeline (conv_tn_pipe.h) with the temporal tap in the operand gather: pixel-major operands, a k-tile =
// 32 consecutive output positions, LDS images [32][BM] / [32][BN] bf16 filled by `buffer_load_dwordx4 ... lds` with
// the XOR swizzle on the source chunk, NST-stage ring, ds_read_b64_tr_b16 fragments.  Each lane owns one fixed patch
// column block (kt, r, s, c..c+7); a position is (frame, oh, ow) with frame = n*T + t, and the tap (kt, r, s) reads
// frame + kt - pad_t only while 0 <= t + kt - pad_t < T: frames outside a clip contribute zero and the neighbouring
// clip is never read.  Split-K partial tiles ALWAYS go through the fp32 slab in register order and are summed in split
// order by conv3d_wgrad_reduce_kernel, which also transposes [K][(kt,r,s,c)] to the Parameter layout OIDHW
// [K][C][KT][R][S]: no atomics, bitwise-reproducible.
#include "avt_common.h"

namespace avt {

#include "conv_params.h"
#include "conv_epi.h"
#include "conv_nt_pipe.h"
#include "conv_tn_pipe.h"  // tn_swz

struct Wgrad3dParams {
  const bf16_t* dy;  // [Kred][Mg]
  const bf16_t* x;   // [N*T][H][W][Cp]
  float* slab;       // [splits][tiles][wave][i][j][quarter][64 lanes] float4
  int Mg, Ng, Kred;  // filters, padded patch width (multiple of BN), N*T*P*Q
  int T, H, W, Cp, P, Q, KT, R, S, stride, pad_t, pad;
  int kt_per_split;
  MagicDiv div_pq, div_q, div_t;
  unsigned dy_bytes, x_bytes;
};

template <int WM, int WN, int TM, int TN, int NST>
__global__ __launch_bounds__(WM * WN * 64) void conv3d_wgrad_kernel(Wgrad3dParams p) {
  constexpr int NW = WM * WN;
  static_assert(NW == 4, "4 waves");
  constexpr int BM = WM * TM * 32, BN = WN * TN * 32;
  constexpr int AROWB = BM * 2, BROWB = BN * 2;
  constexpr int A_RPI = 1024 / AROWB, B_RPI = 1024 / BROWB;
  constexpr int AI = 32 / A_RPI / NW, BI = 32 / B_RPI / NW;
  static_assert(AI >= 1 && BI >= 1 && AI * A_RPI * NW == 32 && BI * B_RPI * NW == 32, "tile/wave split");
  constexpr int LPT = AI + BI;
  constexpr int A_BYTES = 32 * AROWB, STAGE = 32 * (AROWB + BROWB);
  __shared__ __attribute__((aligned(16))) char smem[NST * STAGE];

  const int tid = threadIdx.x, lane = tid & 63;
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wid / WN, wn = wid % WN;
  const int nnt = p.Ng / BN;
  const int ntiles = (p.Mg / BM) * nnt;
  const int lin = xcd_remap(blockIdx.x, gridDim.x);
  const int split = lin / ntiles, tile = lin - split * ntiles;
  const int mt = tile / nnt, nt = tile - mt * nnt;
  const int m0 = mt * BM, n0 = nt * BN;
  const int nkt_total = (p.Kred + 31) / 32;
  const int kt_begin = split * p.kt_per_split;
  const int kt_end = min(nkt_total, kt_begin + p.kt_per_split);  // the host's split count leaves no range empty
  const int nkt = kt_end - kt_begin;

  const __amdgpu_buffer_rsrc_t rsa = __builtin_amdgcn_make_buffer_rsrc((void*)p.dy, (short)0, (int)p.dy_bytes, 0x00020000);
  const __amdgpu_buffer_rsrc_t rsb = __builtin_amdgcn_make_buffer_rsrc((void*)p.x, (short)0, (int)p.x_bytes, 0x00020000);

  const int a_r = lane / (AROWB / 16), a_pc = lane % (AROWB / 16);
  const int b_r = lane / (BROWB / 16), b_pc = lane % (BROWB / 16);

  const int sh = p.stride - 1;
  const unsigned rowB = (unsigned)(p.W * p.Cp * 2), pixB = (unsigned)(p.Cp * 2);
  const unsigned imgB = (unsigned)(p.H * p.W * p.Cp * 2);  // one frame
  const int step_oh = 32 / p.Q, step_ow = 32 - (32 / p.Q) * p.Q;
  const bool tiny = p.P * p.Q < 32;
  int b_oh[BI], b_ow[BI], b_t[BI], y_off[BI], x_off[BI], t_off[BI];
  unsigned b_fb[BI], cB[BI];
#pragma unroll
  for (int i = 0; i < BI; ++i) {
    const int row = (wid * BI + i) * B_RPI + b_r;
    const int col = n0 + (b_pc ^ tn_swz<BROWB>(row)) * 8;  // (kt, r, s, c) patch column of this lane
    const int tap = col / p.Cp;
    const int b_c = col - tap * p.Cp;
    const int b_ss = tap % p.S, b_rr = (tap / p.S) % p.R, b_kt = tap / (p.S * p.R);
    const bool colok = col < p.KT * p.R * p.S * p.Cp;
    y_off[i] = b_rr - p.pad;
    x_off[i] = colok ? b_ss - p.pad : (1 << 20);  // a column past KT*R*S*C: always out of the image
    t_off[i] = b_kt - p.pad_t;
    // the tap's frame displacement and channel, folded into one byte offset (wraps for a negative displacement; such an
    // offset is used only where the clip predicate holds, and then the sum is back in range)
    cB[i] = (unsigned)(b_c * 2) + (unsigned)t_off[i] * imgB;
    const int pix = kt_begin * 32 + row;
    const unsigned f = magic_div((unsigned)pix, p.div_pq);  // frame n*T + t
    const unsigned rem = (unsigned)pix - f * (unsigned)(p.P * p.Q);
    const unsigned oh = magic_div(rem, p.div_q);
    b_oh[i] = (int)oh;
    b_ow[i] = (int)(rem - oh * (unsigned)p.Q);
    b_fb[i] = f * imgB;
    b_t[i] = (int)(f - magic_div(f, p.div_t) * (unsigned)p.T);
  }
  unsigned a_off[AI];
#pragma unroll
  for (int i = 0; i < AI; ++i) {
    const int row = (wid * AI + i) * A_RPI + a_r;
    const unsigned a_coff = (unsigned)((m0 + (a_pc ^ tn_swz<AROWB>(row)) * 8) * 2);
    a_off[i] = (unsigned)(kt_begin * 32 + row) * (unsigned)(p.Mg * 2) + a_coff;
  }
  const unsigned a_step = 32u * (unsigned)(p.Mg * 2);

  const unsigned smem_lds = (unsigned)(size_t)(lds_void_t*)smem;
  auto issue = [&](int kt, int stage) {  // tiles are issued in order; kt past the end is a dummy
    const unsigned As = smem_lds + (unsigned)(stage * STAGE);
    const unsigned Bs = As + A_BYTES;
    const bool live = kt < kt_end;
    // positions past the batch (the last tile): their DY rows lie past the buffer (zeros), and their frames -- N*T
    // and up, t counted on -- pass the clip predicate only for frames that are past the buffer too
    const unsigned Hl = live ? (unsigned)p.H : 0u;
#pragma unroll
    for (int i = 0; i < AI; ++i) {
      buf_lds16_at(rsa, As + (unsigned)((wid * AI + i) * 1024), live ? a_off[i] : kOOB);
      a_off[i] += a_step;
    }
#pragma unroll
    for (int i = 0; i < BI; ++i) {
      const int y = (b_oh[i] << sh) + y_off[i], x = (b_ow[i] << sh) + x_off[i];
      const bool ok = (unsigned)y < Hl && (unsigned)x < (unsigned)p.W && (unsigned)(b_t[i] + t_off[i]) < (unsigned)p.T;
      const unsigned off = b_fb[i] + __umul24((unsigned)y, rowB) + __umul24((unsigned)x, pixB) + cB[i];
      buf_lds16_at(rsb, Bs + (unsigned)((wid * BI + i) * 1024), ok ? off : kOOB);
      int ow = b_ow[i] + step_ow, oh = b_oh[i] + step_oh;
      const bool wr = ow >= p.Q;
      ow = wr ? ow - p.Q : ow;
      oh = wr ? oh + 1 : oh;
      if (!tiny) {
        const bool nx = oh >= p.P;  // next frame
        b_oh[i] = nx ? oh - p.P : oh;
        b_fb[i] = nx ? b_fb[i] + imgB : b_fb[i];
        const int tn = nx ? b_t[i] + 1 : b_t[i];
        b_t[i] = tn >= p.T ? tn - p.T : tn;
      } else {  // frames of fewer than 32 positions: several per tile (uniform branch)
        while (oh >= p.P) {
          oh -= p.P;
          b_fb[i] += imgB;
          b_t[i] = b_t[i] + 1 >= p.T ? 0 : b_t[i] + 1;
        }
        b_oh[i] = oh;
      }
      b_ow[i] = ow;
    }
  };

  f32x16 acc[TM][TN];
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j)
#pragma unroll
      for (int v = 0; v < 16; ++v) acc[i][j][v] = 0.f;

  const int g = lane >> 4, t = lane & 15, q = t >> 2, pq = t & 3;
  const int tr_row = (g >> 1) * 8 + q;
  const int tr_col = (g & 1) * 16 + 4 * pq;
  const int a_sw = tn_swz<AROWB>(q), b_sw = tn_swz<BROWB>(q);
  typedef __attribute__((address_space(3))) s16x4 lds_s16x4;

#pragma unroll
  for (int s = 0; s < NST - 1; ++s) issue(kt_begin + s, s);

  bf16x8 af[2][TM], bfr[2][TN];
  auto load_frags = [&](const char* As, const char* Bs, int ks, int buf) {
#pragma unroll
    for (int i = 0; i < TM; ++i) {
      const int c = wm * (BM / WM) + i * 32 + tr_col;
      const int off = ((c >> 3) ^ a_sw) * 16 + (c & 7) * 2;
      const char* a0 = As + (ks * 16 + tr_row) * AROWB + off;
      s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)(a0));
      s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)(a0 + 4 * AROWB));
      af[buf][i] = __builtin_bit_cast(bf16x8, __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7));
    }
#pragma unroll
    for (int j = 0; j < TN; ++j) {
      const int c = wn * (BN / WN) + j * 32 + tr_col;
      const int off = ((c >> 3) ^ b_sw) * 16 + (c & 7) * 2;
      const char* b0 = Bs + (ks * 16 + tr_row) * BROWB + off;
      s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)(b0));
      s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)(b0 + 4 * BROWB));
      bfr[buf][j] = __builtin_bit_cast(bf16x8, __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7));
    }
  };
  auto mma = [&](int buf) {
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
      for (int j = 0; j < TN; ++j)
        acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af[buf][i], bfr[buf][j], acc[i][j], 0, 0, 0);
  };
  auto step = [&](int k, int rs, int is) {  // rs: the stage read, is: the stage the DMA issued here fills
    wait_vmcnt<(NST - 2) * LPT>();
    ring_barrier();
    const char* As = smem + rs * STAGE;
    const char* Bs = As + A_BYTES;
    load_frags(As, Bs, 0, 0);
    issue(kt_begin + k + NST - 1, is);
    load_frags(As, Bs, 1, 1);
    __builtin_amdgcn_sched_barrier(0);
    mma(0);
    __builtin_amdgcn_sched_barrier(0);
    mma(1);
  };
  for (int k0 = 0; k0 < nkt; k0 += NST) {
#pragma unroll
    for (int u = 0; u < NST; ++u)
      if (k0 + u < nkt) step(k0 + u, u, (u + NST - 1) % NST);
  }
  wait_vmcnt<0>();

  // the partial tile to the slab in register order: [split][tile][wave][i][j][quarter] x 64 lanes x 16 B
  f32x4* dst = reinterpret_cast<f32x4*>(p.slab) + ((size_t)(split * ntiles + tile) * NW + wid) * (TM * TN * 4 * 64) + lane;
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j)
#pragma unroll
      for (int qq = 0; qq < 4; ++qq)
        dst[((i * TN + j) * 4 + qq) * 64] =
            f32x4{acc[i][j][4 * qq], acc[i][j][4 * qq + 1], acc[i][j][4 * qq + 2], acc[i][j][4 * qq + 3]};
}

// DW (OIDHW [K][C][taps]) += sum over the splits, in split order, of the register-order partial tiles: one thread
// per float4 slab position, a position's splits 8 loads at a time; the position's GEMM column (tap, c) is stored at
// its Parameter place (k*C + c)*taps + tap.
__global__ __launch_bounds__(256) void conv3d_wgrad_reduce_kernel(const float* __restrict__ slab, int splits, int ntiles,
                                                                  int nnt, int Mg, int C, int taps, int WM, int WN,
                                                                  int TM, int TN, float* __restrict__ dw) {
  const int NW = WM * WN, BM = WM * TM * 32, BN = WN * TN * 32;
  const long long total = (long long)ntiles * NW * TM * TN * 4 * 64;
  const f32x4* s4 = reinterpret_cast<const f32x4*>(slab);
  for (long long f = (long long)blockIdx.x * 256 + threadIdx.x; f < total; f += (long long)gridDim.x * 256) {
    f32x4 a = {0.f, 0.f, 0.f, 0.f};
    for (int s0 = 0; s0 < splits; s0 += 8) {
      f32x4 v[8];
#pragma unroll
      for (int i = 0; i < 8; ++i) v[i] = s0 + i < splits ? s4[f + (s0 + i) * total] : f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int i = 0; i < 8; ++i) a += v[i];
    }
    const int lane = (int)(f & 63);
    long long r = f >> 6;
    const int q = (int)(r & 3);
    r >>= 2;
    const int jj = (int)(r % TN);
    r /= TN;
    const int i = (int)(r % TM);
    r /= TM;
    const int wid = (int)(r % NW);
    const int tile = (int)(r / NW);
    const int mt = tile / nnt, nt = tile - mt * nnt;
    const int wm = wid / WN, wn = wid % WN;
    const int col = nt * BN + wn * (BN / WN) + jj * 32 + (lane & 31);
    const int r0 = mt * BM + wm * (BM / WM) + i * 32 + 8 * q + 4 * (lane >> 5);
    if (col < taps * C) {
      const int tap = col / C, c = col - tap * C;
#pragma unroll
      for (int e = 0; e < 4; ++e)
        if (r0 + e < Mg) dw[((size_t)(r0 + e) * C + c) * taps + tap] += a[e];
    }
  }
}

struct Wgrad3dPlan {
  Wgrad3dParams p;
  int BM, tiles, splits;
  size_t slab_bytes;
};

static int wgrad3d_cus() {
  static int n = 0;
  if (n == 0) {
    int dev = 0;
    hipDeviceProp_t prop;
    n = (hipGetDevice(&dev) == hipSuccess && hipGetDeviceProperties(&prop, dev) == hipSuccess &&
         prop.multiProcessorCount > 0)
            ? prop.multiProcessorCount
            : 256;
  }
  return n;
}

static inline int conv3d_out(int in, int k, int st, int pad) { return (in + 2 * pad - k) / st + 1; }

// 64- or 128-filter x 128-column tiles; splits so that the grid reaches about two blocks per CU while a block keeps
// at least 8 k-tiles (256 positions); every split's range is non-empty
static Wgrad3dPlan wgrad3d_plan(int N, int T, int H, int W, int Cp, int K, int KT, int R, int S, int stride, int pad_t,
                                int pad) {
  Wgrad3dPlan pl{};
  Wgrad3dParams& p = pl.p;
  p.Mg = K;
  p.T = T; p.H = H; p.W = W; p.Cp = Cp;
  p.P = conv3d_out(H, R, stride, pad);
  p.Q = conv3d_out(W, S, stride, pad);
  p.KT = KT; p.R = R; p.S = S; p.stride = stride; p.pad_t = pad_t; p.pad = pad;
  p.Kred = N * T * p.P * p.Q;
  const int ncols = KT * R * S * Cp;
  p.Ng = (ncols + 127) / 128 * 128;
  pl.BM = K % 128 == 0 ? 128 : 64;
  pl.tiles = (K / pl.BM) * (p.Ng / 128);
  const int nkt = (p.Kred + 31) / 32;
  int splits = 2 * wgrad3d_cus() / pl.tiles;
  if (splits > nkt / 8) splits = nkt / 8;
  if (splits < 1) splits = 1;
  const int kps = (nkt + splits - 1) / splits;
  p.kt_per_split = kps;
  pl.splits = (nkt + kps - 1) / kps;
  pl.slab_bytes = (size_t)pl.splits * p.Mg * p.Ng * sizeof(float);
  return pl;
}

}  // namespace avt

using namespace avt;

static bool wgrad3d_args_ok(int N, int T, int H, int W, int Cp, int K, int KT, int R, int S, int stride, int pad_t,
                            int pad) {
  if (N < 1 || T < 1 || H < 1 || W < 1 || Cp < 32 || Cp % 32 != 0 || K < 64 || K % 64 != 0) return false;
  if (KT < 1 || R < 1 || S < 1 || KT * R * S > kMaxTaps || (stride != 1 && stride != 2) || pad_t < 0 || pad < 0)
    return false;
  if (T + 2 * pad_t - KT + 1 != T) return false;  // temporal 'same' (the R3D-18's 3x3x3 / pad 1 and 1x1x1 / pad 0)
  return conv3d_out(H, R, stride, pad) >= 1 && conv3d_out(W, S, stride, pad) >= 1;
}

extern "C" size_t avt_conv3d_wgrad_workspace(int N, int T, int H, int W, int Cp, int K, int KT, int R, int S,
                                             int stride, int pad_t, int pad) {
  if (!wgrad3d_args_ok(N, T, H, W, Cp, K, KT, R, S, stride, pad_t, pad)) return 0;
  return wgrad3d_plan(N, T, H, W, Cp, K, KT, R, S, stride, pad_t, pad).slab_bytes;
}

// dw fp32 OIDHW [K][Cp][KT][R][S] += wgrad(x [N][T][H][W][Cp], dy [N][T][P][Q][K]); the workspace is required
// (every partial goes through the slab: there is no atomic path)
extern "C" int avt_conv3d_wgrad(const void* x, const void* dy, float* dw, int N, int T, int H, int W, int Cp, int K,
                                int KT, int R, int S, int stride, int pad_t, int pad, void* workspace, size_t ws_bytes,
                                void* stream) {
  AVT_REQUIRE(x && dy && dw, "conv3d_wgrad: null pointer");
  AVT_REQUIRE(wgrad3d_args_ok(N, T, H, W, Cp, K, KT, R, S, stride, pad_t, pad),
              "conv3d_wgrad: N=%d T=%d H=%d W=%d C=%d K=%d taps %dx%dx%d stride %d pad %d/%d unsupported (C %% 32, K %% "
              "64, <= %d taps, stride 1 or 2, temporal 'same' padding)",
              N, T, H, W, Cp, K, KT, R, S, stride, pad_t, pad, kMaxTaps);
  Wgrad3dPlan pl = wgrad3d_plan(N, T, H, W, Cp, K, KT, R, S, stride, pad_t, pad);
  AVT_REQUIRE(workspace != nullptr && ws_bytes >= pl.slab_bytes,
              "conv3d_wgrad: needs a workspace of avt_conv3d_wgrad_workspace() = %zu bytes (deterministic split-K "
              "slab; there is no atomic path), got %zu",
              pl.slab_bytes, workspace ? ws_bytes : (size_t)0);
  AVT_REQUIRE(((uintptr_t)workspace & 15) == 0, "conv3d_wgrad: the workspace must be 16-byte aligned");
  Wgrad3dParams& p = pl.p;
  const size_t xb = (size_t)N * T * H * W * Cp * 2, yb = (size_t)p.Kred * K * 2;
  // (the last tile's positions past the batch reach up to 32 + KT frames past the end: still no 32-bit wrap)
  AVT_REQUIRE(xb + (size_t)H * W * Cp * 2 * (KT + 34) < (1ull << 31) && yb + 64ull * K * 2 < (1ull << 31),
              "conv3d_wgrad: activation tensors must stay below 2 GiB (32-bit buffer offsets)");
  AVT_REQUIRE((size_t)W * Cp * 2 < (1u << 24) && H < (1 << 23), "conv3d_wgrad: image row too long");
  p.dy = (const bf16_t*)dy;
  p.x = (const bf16_t*)x;
  p.slab = (float*)workspace;
  p.div_pq = make_magic((unsigned)(p.P * p.Q));
  p.div_q = make_magic((unsigned)p.Q);
  p.div_t = make_magic((unsigned)T);
  p.dy_bytes = (unsigned)yb;
  p.x_bytes = (unsigned)xb;
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid(pl.tiles * pl.splits);
  if (pl.BM == 128)
    hipLaunchKernelGGL((conv3d_wgrad_kernel<2, 2, 2, 2, 4>), grid, dim3(256), 0, st, p);
  else
    hipLaunchKernelGGL((conv3d_wgrad_kernel<2, 2, 1, 2, 4>), grid, dim3(256), 0, st, p);
  const int tm = pl.BM == 128 ? 2 : 1;
  const long long positions = (long long)pl.tiles * 4 * tm * 2 * 4 * 64;
  long long blocks = (positions + 255) / 256;
  if (blocks > 4096) blocks = 4096;
  hipLaunchKernelGGL(conv3d_wgrad_reduce_kernel, dim3((unsigned)blocks), dim3(256), 0, st, (const float*)workspace,
                     pl.splits, pl.tiles, p.Ng / 128, K, Cp, KT * R * S, 2, 2, tm, 2, dw);
  return check_launch("conv3d_wgrad");
}
