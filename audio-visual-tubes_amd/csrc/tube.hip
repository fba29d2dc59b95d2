// Layout kernels of the 3-D tube path (FullModel, model.py:17-36; R3D-18 = models/resnet3D.py).
//
//  * Video stem as a 2-D conv.  The R3D stem Conv3d(3, 64, (7,7,7), stride (1,2,2), pad (3,3,3))
//    (resnet3D.py:122-127) has temporal stride 1, so folding its 7 temporal taps into channels,
//      X'[n][t][h][w][kt*4 + c] = x[n][c][t + kt - 3][h][w]   (0 outside the clip, c = 3 and
//                                                              channels 28..31 zero),
//    turns it into a Conv2d 7x7/s2/p3 with 32 channels over the N*T frames, which runs on the
//    same LDS-DMA MFMA kernel as every other conv (C % 32 == 0).  The weight is packed to match:
//      W'[k][(r*7 + s)*32 + kt*4 + c] = w[k][c][kt][r][s].
//  * Conv3d weight packing: fp32 OIDHW (the Parameter layout) -> bf16 [K][(kt,r,s,c)], the fwd
//    operand of avt_conv3d_fwd.
#include "avt_common.h"

namespace avt {

// one thread per output pixel (n, t, h, w): 32 channels = 64 contiguous bytes
__global__ __launch_bounds__(256) void video_stem_im2col_kernel(const float* __restrict__ x, bf16_t* __restrict__ out,
                                                                int N, int C, int T, int HW, int KT, int pad_t) {
  const long long npix = (long long)N * T * HW;
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < npix;
       i += (long long)gridDim.x * blockDim.x) {
    const int hw = (int)(i % HW);
    const long long nt = i / HW;
    const int t = (int)(nt % T), n = (int)(nt / T);
    float v[32];
#pragma unroll
    for (int j = 0; j < 32; ++j) v[j] = 0.f;
#pragma unroll
    for (int kt = 0; kt < 8; ++kt) {
      if (kt >= KT) break;
      const int tt = t + kt - pad_t;
      if (tt < 0 || tt >= T) continue;
#pragma unroll
      for (int c = 0; c < 4; ++c)
        if (c < C) v[kt * 4 + c] = x[(((long long)n * C + c) * T + tt) * HW + hw];
    }
    u32x4* o = reinterpret_cast<u32x4*>(out + i * 32);
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      u32x4 w;
      w[0] = pack2(v[q * 8 + 0], v[q * 8 + 1]);
      w[1] = pack2(v[q * 8 + 2], v[q * 8 + 3]);
      w[2] = pack2(v[q * 8 + 4], v[q * 8 + 5]);
      w[3] = pack2(v[q * 8 + 6], v[q * 8 + 7]);
      o[q] = w;
    }
  }
}

// fold = 0: out[k][((kt*R + r)*S + s)*C + c] = w[k][c][kt][r][s]            (Kg = KT*R*S*C)
// fold = 1: out[k][(r*S + s)*32 + kt*4 + c] = w[k][c][kt][r][s], zero padded (Kg = R*S*32)
__global__ __launch_bounds__(256) void pack_conv3d_kernel(const float* __restrict__ w, bf16_t* __restrict__ out, int K,
                                                          int C, int KT, int R, int S, int fold, long long total) {
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total;
       i += (long long)gridDim.x * blockDim.x) {
    const int kg = fold ? R * S * 32 : KT * R * S * C;
    const int k = (int)(i / kg), j = (int)(i % kg);
    int kt, r, s, c;
    bool ok = true;
    if (fold) {
      const int rs = j / 32, q = j % 32;
      r = rs / S;
      s = rs % S;
      kt = q / 4;
      c = q % 4;
      ok = kt < KT && c < C;
    } else {
      c = j % C;
      const int t = j / C;
      s = t % S;
      r = (t / S) % R;
      kt = t / (S * R);
    }
    const float v = ok ? w[((((long long)k * C + c) * KT + kt) * R + r) * S + s] : 0.f;
    out[i] = f2bf(v);
  }
}

// fold = 0 with the filter row in LDS: out[k] is the (C x T) -> (T x C) transpose of w[k] (T = KT*R*S taps): one block
// per output row, the fp32 row read into LDS with 16-byte loads, the bf16 row written 8 channels (16 bytes) per
// thread (both sides coalesced; the element kernel above reads with a T-float stride).  C % 8 == 0.  Same values as
// pack_conv3d_kernel.
__global__ __launch_bounds__(256) void pack_conv3d_rows_kernel(const float* __restrict__ w, bf16_t* __restrict__ out,
                                                               int K, int C, int T) {
  extern __shared__ __attribute__((aligned(16))) float row[];  // C * T floats
  const int n = C * T;
  for (int k = blockIdx.x; k < K; k += gridDim.x) {
    const float4* src = reinterpret_cast<const float4*>(w + (size_t)k * n);
    __syncthreads();
    for (int i = threadIdx.x; i < n / 4; i += blockDim.x) reinterpret_cast<float4*>(row)[i] = src[i];
    __syncthreads();
    u32x4* dst = reinterpret_cast<u32x4*>(out + (size_t)k * n);
    for (int j = threadIdx.x; j < n / 8; j += blockDim.x) {  // output elements 8j .. 8j + 7: tap t, channels c .. c + 7
      const int t = (8 * j) / C, c = 8 * j - t * C;
      const float* r0 = row + c * T + t;
      u32x4 o;
      o.x = pack2(r0[0], r0[T]);
      o.y = pack2(r0[2 * T], r0[3 * T]);
      o.z = pack2(r0[4 * T], r0[5 * T]);
      o.w = pack2(r0[6 * T], r0[7 * T]);
      dst[j] = o;
    }
  }
}

// Every non-stem Conv3d weight of the R3D trunk in ONE launch (blockIdx.y = conv): the filter-row transpose above per
// descriptor, its element form for a descriptor the 16-byte path cannot take (C % 8 != 0 or misaligned operands).
struct Pack3dDesc {
  const float* w;  // fp32 OIDHW [K][C][T]
  bf16_t* out;     // bf16 [K][T*C]
  int K, C, T, pad_;
};

__global__ __launch_bounds__(256) void pack_conv3d_batched_kernel(const Pack3dDesc* __restrict__ descs) {
  extern __shared__ __attribute__((aligned(16))) float row[];
  const Pack3dDesc d = descs[blockIdx.y];
  const int n = d.C * d.T;
  const bool vec = d.C % 8 == 0 && ((((uintptr_t)d.w) | ((uintptr_t)d.out)) & 15) == 0;
  for (int k = blockIdx.x; k < d.K; k += gridDim.x) {
    const float* wk = d.w + (size_t)k * n;
    bf16_t* ok = d.out + (size_t)k * n;
    if (!vec) {
      for (int j = threadIdx.x; j < n; j += blockDim.x) {
        const int t = j / d.C, c = j - t * d.C;
        ok[j] = f2bf(wk[c * d.T + t]);
      }
      continue;
    }
    __syncthreads();
    for (int i = threadIdx.x; i < n / 4; i += blockDim.x)
      reinterpret_cast<float4*>(row)[i] = reinterpret_cast<const float4*>(wk)[i];
    __syncthreads();
    for (int j = threadIdx.x; j < n / 8; j += blockDim.x) {
      const int t = (8 * j) / d.C, c = 8 * j - t * d.C;
      const float* r0 = row + c * d.T + t;
      u32x4 o;
      o.x = pack2(r0[0], r0[d.T]);
      o.y = pack2(r0[2 * d.T], r0[3 * d.T]);
      o.z = pack2(r0[4 * d.T], r0[5 * d.T]);
      o.w = pack2(r0[6 * d.T], r0[7 * d.T]);
      reinterpret_cast<u32x4*>(ok)[j] = o;
    }
  }
}

// Inference fold of the R3D trunk's frozen BatchNorm3d's into the Conv3d's in front of them (avt_fold_conv3d_bn_batched;
// the 2-D one is misc.hip's fold_conv_bn_batched_kernel): with s[k] = gamma[k] * rsqrt(running_var[k] + eps) (the
// rsqrt taken through fp64, see the kernel),
// bn(conv(x, w)) = conv(x, w * s) + (beta - running_mean * s).  One record per conv, blockIdx.y = record, one block per
// filter row as pack_conv3d_batched_kernel: the fp32 OIDHW row goes through LDS, so reads and writes are both
// contiguous.  The image is that kernel's (fold-0 layout) -- for the stem record pack_conv3d_kernel's fold-1 layout
// [K][(r, s)][kt*4 + c], zero padded -- of w[k, ...] * s[k], the product formed in fp32 and rounded to bf16 once;
// bias[k] = beta[k] - mean[k] * s[k] in two separately rounded operations.  Unlike the 2-D stems, whose BatchNorm stays
// in the fused max-pool kernel, the R3D stem folds like the rest (FullModel's trunk has no max-pool).  Every output
// element is written by one thread from its own inputs: deterministic, no atomics.
struct Fold3dDesc {
  const float* w;      // fp32 OIDHW [K][C][KT][R][S]
  bf16_t* out;         // bf16 [K][KT*R*S*C], or (stem) [K][R*S*32]
  const float* gamma;  // [K]
  const float* beta;
  const float* mean;   // running_mean
  const float* var;    // running_var
  float* bias;         // [K]
  int K, C, KT, R, S, stem;
  float eps;
  int pad_;
};

__global__ __launch_bounds__(256) void fold_conv3d_bn_batched_kernel(const Fold3dDesc* __restrict__ descs) {
#pragma clang fp contract(off)  // beta - mean * s stays two rounded operations (no fma), as documented above
  extern __shared__ __attribute__((aligned(16))) float row[];
  const Fold3dDesc d = descs[blockIdx.y];
  const int RS = d.R * d.S, T = d.KT * RS;
  const int n = d.C * T;
  const bool vec = !d.stem && d.C % 8 == 0 && ((((uintptr_t)d.w) | ((uintptr_t)d.out)) & 15) == 0;
  for (int k = blockIdx.x; k < d.K; k += gridDim.x) {
    // rsqrt through fp64 (sqrt and divide are correctly rounded there, then one rounding back to fp32): a value any
    // IEEE host reproduces bit for bit (tests/test_fold3d_pack_gpu.py does, in torch), which the hardware approximation
    // behind rsqrtf (off by one ulp on about one input in ten) is not
    const float inv = (float)(1.0 / sqrt((double)(d.var[k] + d.eps)));
    const float s = __fmul_rn(d.gamma[k], inv);
    if (threadIdx.x == 0) {  // plain operators: the pragma above covers them (not the bodies of inlined intrinsics)
      const float ms = d.mean[k] * s;
      d.bias[k] = d.beta[k] - ms;
    }
    const float* wk = d.w + (size_t)k * n;
    __syncthreads();  // the previous row has been read
    if (vec) {
      for (int i = threadIdx.x; i < n / 4; i += blockDim.x)
        reinterpret_cast<float4*>(row)[i] = reinterpret_cast<const float4*>(wk)[i];
    } else {
      for (int i = threadIdx.x; i < n; i += blockDim.x) row[i] = wk[i];
    }
    __syncthreads();
    if (d.stem) {  // [(r, s)][kt*4 + c], 32 channels per (r, s)
      bf16_t* ok = d.out + (size_t)k * RS * 32;
      for (int j = threadIdx.x; j < RS * 32; j += blockDim.x) {
        const int rs = j >> 5, q = j & 31;
        const int kt = q >> 2, c = q & 3;
        float v = 0.f;
        if (kt < d.KT && c < d.C) v = __fmul_rn(row[(c * d.KT + kt) * RS + rs], s);
        ok[j] = f2bf(v);
      }
      continue;
    }
    bf16_t* ok = d.out + (size_t)k * n;
    if (!vec) {
      for (int j = threadIdx.x; j < n; j += blockDim.x) {
        const int t = j / d.C, c = j - t * d.C;
        ok[j] = f2bf(__fmul_rn(row[c * T + t], s));
      }
      continue;
    }
    for (int j = threadIdx.x; j < n / 8; j += blockDim.x) {  // tap t, channels c .. c + 7: one 16-byte store
      const int t = (8 * j) / d.C, c = 8 * j - t * d.C;
      const float* r0 = row + c * T + t;
      u32x4 o;
      o.x = pack2(__fmul_rn(r0[0], s), __fmul_rn(r0[T], s));
      o.y = pack2(__fmul_rn(r0[2 * T], s), __fmul_rn(r0[3 * T], s));
      o.z = pack2(__fmul_rn(r0[4 * T], s), __fmul_rn(r0[5 * T], s));
      o.w = pack2(__fmul_rn(r0[6 * T], s), __fmul_rn(r0[7 * T], s));
      reinterpret_cast<u32x4*>(ok)[j] = o;
    }
  }
}

// out[(b*rep + k)][c] = in[b][c]  (the per-clip audio vector of each of its t frames)
__global__ __launch_bounds__(256) void repeat_rows_kernel(const float* __restrict__ in, float* __restrict__ out, int B,
                                                          int rep, int C) {
  const long long n = (long long)B * rep * C;
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
    const int c = (int)(i % C);
    const long long row = i / C;
    out[i] = in[(row / rep) * C + c];
  }
}

// out[b][c] = sum_k in[(b*rep + k)][c]  (adjoint of repeat_rows_kernel)
__global__ __launch_bounds__(256) void sum_rep_rows_kernel(const float* __restrict__ in, float* __restrict__ out, int B,
                                                           int rep, int C) {
  const long long n = (long long)B * C;
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
    const int c = (int)(i % C);
    const long long b = i / C;
    float a = 0.f;
    for (int k = 0; k < rep; ++k) a += in[(b * rep + k) * C + c];
    out[i] = a;
  }
}

// MaxPool3d(kernel_size=3, stride=2, padding=1) (resnet3D.py:129, applied after the stem's BN + ReLU when
// no_max_pool=False, :200-201) over bf16 NDHWC [N][T][H][W][C] -> [N][To][Ho][Wo][C], To = (T - 1) / 2 + 1 (same
// for H, W).  One thread per output pixel and 8 channels (16 B loads of the 27 taps); taps outside the clip are
// skipped (torch's -inf padding); the result is the winning input's bits, and a NaN tap wins, as in max_pool3d.
__global__ __launch_bounds__(256) void maxpool3d_k3s2p1_kernel(const bf16_t* __restrict__ x, bf16_t* __restrict__ y,
                                                               int N, int T, int H, int W, int C, int To, int Ho,
                                                               int Wo) {
  const int cv = C / 8;
  const long long total = (long long)N * To * Ho * Wo * cv;
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total;
       i += (long long)gridDim.x * blockDim.x) {
    const int c8 = (int)(i % cv);
    long long r = i / cv;
    const int wo = (int)(r % Wo);
    r /= Wo;
    const int ho = (int)(r % Ho);
    r /= Ho;
    const int to = (int)(r % To);
    const int n = (int)(r / To);
    float m[8];
    unsigned short bits[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      m[e] = -__builtin_inff();
      bits[e] = 0xff80;  // -inf (never stored: every window holds at least its centre tap)
    }
    for (int dt = 0; dt < 3; ++dt) {
      const int t = 2 * to - 1 + dt;
      if (t < 0 || t >= T) continue;
      for (int dh = 0; dh < 3; ++dh) {
        const int h = 2 * ho - 1 + dh;
        if (h < 0 || h >= H) continue;
        for (int dw = 0; dw < 3; ++dw) {
          const int w = 2 * wo - 1 + dw;
          if (w < 0 || w >= W) continue;
          const u32x4 v = reinterpret_cast<const u32x4*>(x)[(((long long)n * T + t) * H + h) * (long long)W * cv +
                                                           (long long)w * cv + c8];
#pragma unroll
          for (int e = 0; e < 8; ++e) {
            const unsigned short b = (unsigned short)((e & 1) ? (v[e >> 1] >> 16) : (v[e >> 1] & 0xffff));
            const float f = bf2f(b);
            if (f > m[e] || f != f) {
              if (m[e] == m[e]) {  // a NaN already taken stays
                m[e] = f;
                bits[e] = b;
              }
            }
          }
        }
      }
    }
    u32x4 o;
#pragma unroll
    for (int q = 0; q < 4; ++q) o[q] = (unsigned)bits[2 * q] | ((unsigned)bits[2 * q + 1] << 16);
    reinterpret_cast<u32x4*>(y)[i] = o;
  }
}

// Conv3d dgrad operand: out[c][tf*K + k] = bf16(w[k][c][T-1-tf]) (T = KT*R*S taps; the linear flip reverses kt, r and s
// at once) -- the fold-0 layout with K and C swapped and the taps reversed, so that the stride-1 input gradient is
// avt_conv3d_fwd's own conv of dy.  One block per (c, 64 filters): the 64 tap runs of w read through LDS, 128-byte
// bf16 runs written.  K % 64 == 0, T <= 64.
__device__ __forceinline__ void pack_conv3d_dgrad_tile(const float* __restrict__ w, bf16_t* __restrict__ out, int K,
                                                       int C, int T, int blk, float* tile) {
  const int kb = K / 64;
  const int c = blk / kb, k0 = (blk - c * kb) * 64;
  __syncthreads();
  for (int i = threadIdx.x; i < 64 * T; i += blockDim.x) {
    const int kk = i / T, t = i - kk * T;
    tile[i] = w[((size_t)(k0 + kk) * C + c) * T + t];
  }
  __syncthreads();
  for (int i = threadIdx.x; i < 64 * T; i += blockDim.x) {
    const int tf = i >> 6, kk = i & 63;
    out[((size_t)c * T + tf) * K + k0 + kk] = f2bf(tile[kk * T + (T - 1 - tf)]);
  }
}

__global__ __launch_bounds__(256) void pack_conv3d_dgrad_kernel(const float* __restrict__ w, bf16_t* __restrict__ out,
                                                                int K, int C, int T) {
  __shared__ float tile[64 * 64];
  const int nblk = C * (K / 64);
  for (int b = blockIdx.x; b < nblk; b += gridDim.x) pack_conv3d_dgrad_tile(w, out, K, C, T, b, tile);
}

// the same for every record of a Pack3dDesc table in one launch (blockIdx.y = conv; out = that conv's dgrad operand)
__global__ __launch_bounds__(256) void pack_conv3d_dgrad_batched_kernel(const Pack3dDesc* __restrict__ descs) {
  __shared__ float tile[64 * 64];
  const Pack3dDesc d = descs[blockIdx.y];
  const int nblk = d.C * (d.K / 64);
  for (int b = blockIdx.x; b < nblk; b += gridDim.x) pack_conv3d_dgrad_tile(d.w, d.out, d.K, d.C, d.T, b, tile);
}

// Backward of maxpool3d_k3s2p1_kernel in gather form (no atomics): one thread per INPUT voxel and 8 channels sums the
// gy of the (at most 2 x 2 x 2) windows that hold it and whose winner it is.  The winner is recomputed from x as the
// forward takes it: the first maximum in (t, h, w) scan order (a NaN tap wins and stays) -- torch's CPU max_pool3d
// choice, which decides where the gradient of the ReLU output's all-zero windows goes.  fp32 sum, one bf16 rounding.
__global__ __launch_bounds__(256) void maxpool3d_k3s2p1_bwd_kernel(const bf16_t* __restrict__ gy,
                                                                   const bf16_t* __restrict__ x,
                                                                   bf16_t* __restrict__ gx, int N, int T, int H, int W,
                                                                   int C, int To, int Ho, int Wo) {
  const int cv = C / 8;
  const long long total = (long long)N * T * H * W * cv;
  const u32x4* x4 = reinterpret_cast<const u32x4*>(x);
  const u32x4* g4 = reinterpret_cast<const u32x4*>(gy);
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total;
       i += (long long)gridDim.x * blockDim.x) {
    const int c8 = (int)(i % cv);
    long long r = i / cv;
    const int w = (int)(r % W);
    r /= W;
    const int h = (int)(r % H);
    r /= H;
    const int t = (int)(r % T);
    const int n = (int)(r / T);
    float sum[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) sum[e] = 0.f;
    // windows holding coordinate v: o with 2o - 1 <= v <= 2o + 1
    for (int to = t / 2; to <= (t + 1) / 2 && to < To; ++to)
      for (int ho = h / 2; ho <= (h + 1) / 2 && ho < Ho; ++ho)
        for (int wo = w / 2; wo <= (w + 1) / 2 && wo < Wo; ++wo) {
          float m[8];
          int win[8];  // the winner's tap index (dt * 3 + dh) * 3 + dw
#pragma unroll
          for (int e = 0; e < 8; ++e) {
            m[e] = -__builtin_inff();
            win[e] = -1;
          }
          for (int dt = 0; dt < 3; ++dt) {
            const int tt = 2 * to - 1 + dt;
            if (tt < 0 || tt >= T) continue;
            for (int dh = 0; dh < 3; ++dh) {
              const int hh = 2 * ho - 1 + dh;
              if (hh < 0 || hh >= H) continue;
              for (int dw = 0; dw < 3; ++dw) {
                const int ww = 2 * wo - 1 + dw;
                if (ww < 0 || ww >= W) continue;
                const u32x4 v = x4[((((long long)n * T + tt) * H + hh) * W + ww) * cv + c8];
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                  const float f = bf2f((bf16_t)((e & 1) ? (v[e >> 1] >> 16) : (v[e >> 1] & 0xffff)));
                  if ((f > m[e] || f != f) && m[e] == m[e]) {
                    m[e] = f;
                    win[e] = (dt * 3 + dh) * 3 + dw;
                  }
                }
              }
            }
          }
          const int mine = ((t - 2 * to + 1) * 3 + (h - 2 * ho + 1)) * 3 + (w - 2 * wo + 1);
          const u32x4 g = g4[((((long long)n * To + to) * Ho + ho) * Wo + wo) * cv + c8];
#pragma unroll
          for (int e = 0; e < 8; ++e)
            if (win[e] == mine) sum[e] += bf2f((bf16_t)((e & 1) ? (g[e >> 1] >> 16) : (g[e >> 1] & 0xffff)));
        }
    u32x4 o;
#pragma unroll
    for (int q = 0; q < 4; ++q) o[q] = pack2(sum[2 * q], sum[2 * q + 1]);
    reinterpret_cast<u32x4*>(gx)[i] = o;
  }
}

// dw[k][c][kt][r][s] += dwf[k][r][s][kt*4 + c]: the folded stem's 2-D weight gradient (32 channels per (r, s), the
// layout of avt_pack_conv3d_weight fold 1) back to the Parameter's OIDHW layout
__global__ __launch_bounds__(256) void stem3d_wgrad_unfold_kernel(const float* __restrict__ dwf, float* __restrict__ dw,
                                                                  int K, int C, int KT, int R, int S) {
  const int total = K * C * KT * R * S;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < total; i += gridDim.x * blockDim.x) {
    int j = i;
    const int s = j % S;
    j /= S;
    const int r = j % R;
    j /= R;
    const int kt = j % KT;
    j /= KT;
    const int c = j % C, k = j / C;
    dw[i] += dwf[((size_t)(k * R + r) * S + s) * 32 + kt * 4 + c];
  }
}

// ---- input gradient of the R3D stem Conv3d(3, 64, (7,7,7), stride (1,2,2), pad 3) (resnet3D.py:122-127) ----
//   gx[n][c][tau][h][w] = sum_{kt, r, s, k} gy[n][tau - kt + 3][(h + 3 - r) / 2][(w + 3 - s) / 2][k] * w[k][c][kt][r][s]
// over the frames inside the clip and the (r, s) of the voxel's (h % 2, w % 2) parity class whose output position
// falls inside the P x Q map: 3 or 4 rows times 3 or 4 columns of the 7 x 7.  Both forms launch one block range per
// class (the classes with the most taps first), blockIdx.y = the clip: a block never spans two clips.
struct VsdArgs {
  const bf16_t* gy;  // [N][T][P][Q][64]
  const float* w;    // form 0: fp32 OIDHW [64][3][7][7][7]
  const u32x4* wp;   // form 1: avt_pack_video_stem_dgrad's operand
  float* gx;         // [N][3][T][H][W]
  int T, H, W, P, Q;
  int first[5];      // block range [first[i], first[i + 1]) of launch class i
  int cls[4];        // its (h % 2) * 2 + (w % 2)
};

struct VsdClass {
  int ph, pw, Wc, Mc, r0, s0, nr, ns, blk;
};

__device__ __forceinline__ VsdClass vsd_class(const VsdArgs& a) {
  int ci = 0;
  while (ci < 3 && (int)blockIdx.x >= a.first[ci + 1]) ++ci;
  VsdClass c;
  c.ph = a.cls[ci] >> 1;
  c.pw = a.cls[ci] & 1;
  c.Wc = (a.W - c.pw + 1) / 2;
  c.Mc = ((a.H - c.ph + 1) / 2) * c.Wc;
  c.r0 = (c.ph + 1) & 1;  // the taps r with h + 3 - r even: r0, r0 + 2, ...
  c.s0 = (c.pw + 1) & 1;
  c.nr = 4 - c.r0;
  c.ns = 4 - c.s0;
  c.blk = (int)blockIdx.x - a.first[ci];
  return c;
}

// Form 0, direct: one thread per voxel (n, tau, h, w) of the block's class; fp32 weights, one temporal tap's class
// taps at a time in LDS ([tap][k][4]); fp32 sums in the fixed order (kt, r, s, k).  The 3-D form of
// stem_dgrad_kernel (misc.hip).
__global__ __launch_bounds__(256) void video_stem_dgrad_direct_kernel(VsdArgs a) {
  __shared__ float ws[16 * 64 * 4];
  const VsdClass c = vsd_class(a);
  const int n = blockIdx.y;
  const int idx = c.blk * 256 + (int)threadIdx.x;
  const bool valid = idx < a.T * c.Mc;
  const int tau = valid ? idx / c.Mc : 0, m = valid ? idx - tau * c.Mc : 0;
  const int hc = m / c.Wc, h = 2 * hc + c.ph, x = 2 * (m - hc * c.Wc) + c.pw;
  float acc[3] = {0.f, 0.f, 0.f};
  for (int kt = 0; kt < 7; ++kt) {
    __syncthreads();
    for (int i = threadIdx.x; i < c.nr * c.ns * 256; i += 256) {
      const int ch = i & 3, k = (i >> 2) & 63, tap = i >> 8;
      const int r = c.r0 + 2 * (tap / c.ns), s = c.s0 + 2 * (tap % c.ns);
      ws[i] = ch < 3 ? a.w[((((size_t)k * 3 + ch) * 7 + kt) * 7 + r) * 7 + s] : 0.f;
    }
    __syncthreads();
    const int t = tau - kt + 3;
    if (!valid || t < 0 || t >= a.T) continue;
    const bf16_t* fr = a.gy + ((size_t)n * a.T + t) * a.P * a.Q * 64;
    for (int ia = 0; ia < c.nr; ++ia) {
      const int p = (h + 3 - (c.r0 + 2 * ia)) >> 1;
      if (p < 0 || p >= a.P) continue;
      for (int ib = 0; ib < c.ns; ++ib) {
        const int q = (x + 3 - (c.s0 + 2 * ib)) >> 1;
        if (q < 0 || q >= a.Q) continue;
        const u32x4* row = reinterpret_cast<const u32x4*>(fr + ((size_t)p * a.Q + q) * 64);
        const float* wt = ws + (ia * c.ns + ib) * 256;
#pragma unroll 2
        for (int k8 = 0; k8 < 8; ++k8) {
          const u32x4 v = row[k8];
          const unsigned* u = reinterpret_cast<const unsigned*>(&v);
#pragma unroll
          for (int e = 0; e < 8; ++e) {
            const float g = bf2f((bf16_t)(e & 1 ? u[e >> 1] >> 16 : u[e >> 1] & 0xffff));
            const float4 wk = *reinterpret_cast<const float4*>(wt + (k8 * 8 + e) * 4);
            acc[0] += g * wk.x;
            acc[1] += g * wk.y;
            acc[2] += g * wk.z;
          }
        }
      }
    }
  }
  if (valid)
    for (int ch = 0; ch < 3; ++ch) a.gx[((((size_t)n * 3 + ch) * a.T + tau) * a.H + h) * a.W + x] = acc[ch];
}

// Form 1, MFMA: the transpose of the forward's folded 2-D conv (the file comment).  Per frame t and class,
//   gxf[j = kt*4 + c][pixel] = sum_{(r, s) of the class, k} Wf[j][(r, s, k)] * gy[n][t][p][q][k]
// is a GEMM with 32 rows (21 of them real), 16/12/12/9 x 64 of K and the class's pixels as columns, on
// v_mfma_f32_16x16x32_bf16 with the WEIGHTS as the A operand: lane l then holds, for pixel l & 15, the four channels c
// of temporal tap kt = 4 * jtile + (l >> 4) -- one float4 of the fold-back
//   gx[n][c][t + kt - 3] += gxf[kt*4 + c]
// which is fused: a wave owns kVsdPT tiles of 16 class pixels (consecutive in the class's (h, w) raster) and walks
// the clip's frames in order, adding each frame's eight float4 per lane into its private LDS ring of 8 frames
// [tau & 7][pixel][4]; the seven (kt) lanes of a pixel hit seven different frames, so the adds are plain (no
// atomics) and a voxel's sum runs in the fixed order kt = 6 .. 0.  Frame tau is complete after frame tau + 3 and is
// stored then.  The class's bf16 weights (<= 16 taps x 4 KB of A fragments) stay in LDS for the whole block; the gy
// fragments are 16-byte loads straight from global memory (8 channels of one output pixel per lane; the 2 x 2 taps
// around a pixel re-read it from L1/L2).  No intermediate gxf reaches memory and nothing is rounded to bf16 after
// the operands: fp32 accumulation throughout.
constexpr int kVsdPT = 2, kVsdPix = kVsdPT * 16;
constexpr int kVsdWBytes = 16 * 4096, kVsdLds = kVsdWBytes + 4 * 8 * kVsdPix * 16;

__global__ __launch_bounds__(256) void video_stem_dgrad_mfma_kernel(VsdArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char vsd_smem[];
  const VsdClass c = vsd_class(a);
  const int n = blockIdx.y, lane = threadIdx.x & 63, wave = threadIdx.x >> 6, g = lane >> 4;
  u32x4* wl = reinterpret_cast<u32x4*>(vsd_smem);  // [tap][k half][j tile][lane]
  float4* ring = reinterpret_cast<float4*>(vsd_smem + kVsdWBytes) + wave * 8 * kVsdPix;
  for (int i = threadIdx.x; i < c.nr * c.ns * 256; i += 256) {
    const int tap = i >> 8;
    const int r = c.r0 + 2 * (tap / c.ns), s = c.s0 + 2 * (tap % c.ns);
    wl[i] = a.wp[(r * 7 + s) * 256 + (i & 255)];
  }
  for (int i = lane; i < 8 * kVsdPix; i += 64) ring[i] = make_float4(0.f, 0.f, 0.f, 0.f);
  __syncthreads();
  const int m0 = (c.blk * 4 + wave) * kVsdPix;
  int h[kVsdPT], x[kVsdPT];
  bool ok[kVsdPT];
#pragma unroll
  for (int pt = 0; pt < kVsdPT; ++pt) {
    const int m = m0 + pt * 16 + (lane & 15);
    ok[pt] = m < c.Mc;
    const int hc = ok[pt] ? m / c.Wc : 0;
    h[pt] = 2 * hc + c.ph;
    x[pt] = ok[pt] ? 2 * (m - hc * c.Wc) + c.pw : 0;
  }
  for (int t = 0; t < a.T + 3; ++t) {
    if (t < a.T) {
      f32x4 acc[kVsdPT][2];
#pragma unroll
      for (int pt = 0; pt < kVsdPT; ++pt)
#pragma unroll
        for (int jt = 0; jt < 2; ++jt) acc[pt][jt] = f32x4{0.f, 0.f, 0.f, 0.f};
      const bf16_t* fr = a.gy + ((size_t)n * a.T + t) * a.P * a.Q * 64 + g * 8;
      for (int ia = 0; ia < c.nr; ++ia)
        for (int ib = 0; ib < c.ns; ++ib) {
          const u32x4* src[kVsdPT];
#pragma unroll
          for (int pt = 0; pt < kVsdPT; ++pt) {
            const int p = (h[pt] + 3 - (c.r0 + 2 * ia)) >> 1, q = (x[pt] + 3 - (c.s0 + 2 * ib)) >> 1;
            const bool in = ok[pt] && p >= 0 && p < a.P && q >= 0 && q < a.Q;
            src[pt] = in ? reinterpret_cast<const u32x4*>(fr + ((size_t)p * a.Q + q) * 64) : nullptr;
          }
          const u32x4* wt = wl + (ia * c.ns + ib) * 256 + lane;
#pragma unroll
          for (int kh = 0; kh < 2; ++kh) {
            const bf16x8 a0 = __builtin_bit_cast(bf16x8, wt[(kh * 2 + 0) * 64]);
            const bf16x8 a1 = __builtin_bit_cast(bf16x8, wt[(kh * 2 + 1) * 64]);
#pragma unroll
            for (int pt = 0; pt < kVsdPT; ++pt) {
              const u32x4 bv = src[pt] ? src[pt][kh * 4] : u32x4{0u, 0u, 0u, 0u};  // + 32 channels
              const bf16x8 b = __builtin_bit_cast(bf16x8, bv);
              acc[pt][0] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a0, b, acc[pt][0], 0, 0, 0);
              acc[pt][1] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a1, b, acc[pt][1], 0, 0, 0);
            }
          }
        }
#pragma unroll
      for (int jt = 0; jt < 2; ++jt) {
        const int kt = jt * 4 + g, tau = t + kt - 3;
        if (kt < 7 && tau >= 0 && tau < a.T) {
#pragma unroll
          for (int pt = 0; pt < kVsdPT; ++pt) {
            float4* d = ring + (tau & 7) * kVsdPix + pt * 16 + (lane & 15);
            float4 v = *d;
            v.x += acc[pt][jt][0];
            v.y += acc[pt][jt][1];
            v.z += acc[pt][jt][2];
            *d = v;
          }
        }
      }
    }
    __syncthreads();
    const int tau = t - 3;  // complete: frames tau - 3 .. tau + 3 have been added
    if (tau >= 0) {
      const float* slot = reinterpret_cast<const float*>(ring + (tau & 7) * kVsdPix);
      for (int i = lane; i < 3 * kVsdPix; i += 64) {
        const int ch = i / kVsdPix, px = i - ch * kVsdPix, m = m0 + px;
        if (m < c.Mc) {
          const int hc = m / c.Wc;
          a.gx[((((size_t)n * 3 + ch) * a.T + tau) * a.H + 2 * hc + c.ph) * a.W + 2 * (m - hc * c.Wc) + c.pw] =
              slot[px * 4 + ch];
        }
      }
    }
    __syncthreads();
    if (tau >= 0)
      for (int i = lane; i < kVsdPix; i += 64) ring[(tau & 7) * kVsdPix + i] = make_float4(0.f, 0.f, 0.f, 0.f);
  }
}

// The A fragments of form 1: out[(r*7 + s)][k half][j tile][lane][e] = bf16(w[k][c][kt][r][s]) with
// k = 32 * half + 8 * (lane >> 4) + e and j = 16 * tile + (lane & 15) = kt * 4 + c (zero for kt = 7 and c = 3)
__global__ __launch_bounds__(256) void pack_video_stem_dgrad_kernel(const float* __restrict__ w,
                                                                    bf16_t* __restrict__ out) {
  const int total = 49 * 4 * 64 * 8;
  for (int i = blockIdx.x * 256 + threadIdx.x; i < total; i += gridDim.x * 256) {
    const int e = i & 7, lane = (i >> 3) & 63, jt = (i >> 9) & 1, kh = (i >> 10) & 1, rs = i >> 11;
    const int k = 32 * kh + 8 * (lane >> 4) + e, j = 16 * jt + (lane & 15), kt = j >> 2, ch = j & 3;
    out[i] = f2bf(kt < 7 && ch < 3 ? w[(((size_t)k * 3 + ch) * 7 + kt) * 49 + rs] : 0.f);
  }
}

static int g_video_stem_dgrad = -1;  // -1 = env AVT_VIDEO_STEM_DGRAD (default 1, the MFMA form)
static int video_stem_dgrad_form() {
  if (g_video_stem_dgrad < 0) {
    const char* e = getenv("AVT_VIDEO_STEM_DGRAD");
    g_video_stem_dgrad = e ? (atoi(e) ? 1 : 0) : 1;
  }
  return g_video_stem_dgrad;
}

static int grid_for(long long n) {
  long long g = (n + 255) / 256;
  if (g > 8192) g = 8192;
  return (int)(g < 1 ? 1 : g);
}

}  // namespace avt

using namespace avt;

// x: fp32 NCDHW [N][C][T][H][W] (the reference's frames.float(), train_3D.py:131), C <= 4,
// KT <= 7 -> out: bf16 [N][T][H][W][32] (see the file comment).
extern "C" int avt_video_stem_im2col(const float* x, void* out, int N, int C, int T, int H, int W, int KT, int pad_t,
                                     void* stream) {
  AVT_REQUIRE(x && out, "video_stem_im2col: null pointer");
  AVT_REQUIRE(C >= 1 && C <= 4 && KT >= 1 && KT <= 7, "video_stem_im2col: need C <= 4 and KT <= 7");
  const long long npix = (long long)N * T * H * W;
  if (npix == 0) return AVT_OK;
  hipLaunchKernelGGL(video_stem_im2col_kernel, dim3(grid_for(npix)), dim3(256), 0, (hipStream_t)stream, x,
                     (bf16_t*)out, N, C, T, H * W, KT, pad_t);
  return check_launch("video_stem_im2col");
}

// w: fp32 OIDHW [K][C][KT][R][S] -> out bf16 [K][Kg] (fold: stem layout, Kg = R*S*32)
extern "C" int avt_pack_conv3d_weight(const float* w, void* out, int K, int C, int KT, int R, int S, int fold,
                                      void* stream) {
  AVT_REQUIRE(w && out, "pack_conv3d_weight: null pointer");
  AVT_REQUIRE(!fold || (C <= 4 && KT <= 8), "pack_conv3d_weight: stem fold needs C <= 4, KT <= 8");
  const long long total = (long long)K * (fold ? R * S * 32 : KT * R * S * C);
  const int T = KT * R * S;
  const size_t row_bytes = (size_t)C * T * sizeof(float);
  if (!fold && C % 8 == 0 && row_bytes <= 60 * 1024 && ((((uintptr_t)out) | ((uintptr_t)w)) & 15) == 0) {
    hipLaunchKernelGGL(pack_conv3d_rows_kernel, dim3(K < 2048 ? K : 2048), dim3(256), row_bytes, (hipStream_t)stream, w,
                       (bf16_t*)out, K, C, T);
    return check_launch("pack_conv3d_weight");
  }
  hipLaunchKernelGGL(pack_conv3d_kernel, dim3(grid_for(total)), dim3(256), 0, (hipStream_t)stream, w, (bf16_t*)out, K,
                     C, KT, R, S, fold, total);
  return check_launch("pack_conv3d_weight");
}

// x bf16 [N][T][H][W][C] (C % 8 == 0) -> y bf16 [N][(T-1)/2+1][(H-1)/2+1][(W-1)/2+1][C]: nn.MaxPool3d(3, 2, 1)
extern "C" int avt_maxpool3d_fwd(const void* x, void* y, int N, int T, int H, int W, int C, void* stream) {
  AVT_REQUIRE(x && y, "maxpool3d_fwd: null pointer");
  AVT_REQUIRE(N >= 0 && T >= 1 && H >= 1 && W >= 1 && C >= 8 && C % 8 == 0,
              "maxpool3d_fwd: N=%d T=%d H=%d W=%d C=%d (C a multiple of 8)", N, T, H, W, C);
  const int To = (T - 1) / 2 + 1, Ho = (H - 1) / 2 + 1, Wo = (W - 1) / 2 + 1;
  const long long n = (long long)N * To * Ho * Wo * (C / 8);
  if (n == 0) return AVT_OK;
  hipLaunchKernelGGL(maxpool3d_k3s2p1_kernel, dim3(grid_for(n)), dim3(256), 0, (hipStream_t)stream, (const bf16_t*)x,
                     (bf16_t*)y, N, T, H, W, C, To, Ho, Wo);
  return check_launch("maxpool3d_fwd");
}

// w: fp32 OIDHW [K][C][KT][R][S] -> out bf16 [C][(KT-1-kt, R-1-r, S-1-s, k)]: the operand of avt_conv3d_dgrad
extern "C" int avt_pack_conv3d_weight_dgrad(const float* w, void* out, int K, int C, int KT, int R, int S,
                                            void* stream) {
  AVT_REQUIRE(w && out, "pack_conv3d_weight_dgrad: null pointer");
  AVT_REQUIRE(K >= 64 && K % 64 == 0 && C >= 1 && KT >= 1 && R >= 1 && S >= 1 && KT * R * S <= 64,
              "pack_conv3d_weight_dgrad: K=%d (a multiple of 64), %d taps (<= 64)", K, KT * R * S);
  const int nblk = C * (K / 64);
  hipLaunchKernelGGL(pack_conv3d_dgrad_kernel, dim3(nblk < 8192 ? nblk : 8192), dim3(256), 0, (hipStream_t)stream, w,
                     (bf16_t*)out, K, C, KT * R * S);
  return check_launch("pack_conv3d_weight_dgrad");
}

// descs: device array of n avt_pack3d_desc_bytes() records whose `out` is the conv's dgrad operand [C][T*K] (K % 64
// == 0, T <= 64 -- the caller's to keep: the table is on the device); max_blocks = the largest C * K / 64
extern "C" int avt_pack_conv3d_weights_dgrad_batched(const void* descs, int n, int max_blocks, void* stream) {
  AVT_REQUIRE(descs && n > 0 && max_blocks > 0, "pack_conv3d_weights_dgrad_batched: bad arguments");
  hipLaunchKernelGGL(pack_conv3d_dgrad_batched_kernel, dim3(max_blocks < 2048 ? max_blocks : 2048, n), dim3(256), 0,
                     (hipStream_t)stream, (const Pack3dDesc*)descs);
  return check_launch("pack_conv3d_weights_dgrad_batched");
}

// gx bf16 [N][T][H][W][C] = backward of avt_maxpool3d_fwd(x) under gy bf16 [N][To][Ho][Wo][C]
extern "C" int avt_maxpool3d_bwd(const void* gy, const void* x, const void* y, void* gx, int N, int T, int H, int W,
                                 int C, void* stream) {
  (void)y;  // the winner is recomputed from x (ties: the first maximum), y is not read
  AVT_REQUIRE(gy && x && gx, "maxpool3d_bwd: null pointer");
  AVT_REQUIRE(N >= 0 && T >= 1 && H >= 1 && W >= 1 && C >= 8 && C % 8 == 0,
              "maxpool3d_bwd: N=%d T=%d H=%d W=%d C=%d (C a multiple of 8)", N, T, H, W, C);
  const int To = (T - 1) / 2 + 1, Ho = (H - 1) / 2 + 1, Wo = (W - 1) / 2 + 1;
  const long long n = (long long)N * T * H * W * (C / 8);
  if (n == 0) return AVT_OK;
  hipLaunchKernelGGL(maxpool3d_k3s2p1_bwd_kernel, dim3(grid_for(n)), dim3(256), 0, (hipStream_t)stream,
                     (const bf16_t*)gy, (const bf16_t*)x, (bf16_t*)gx, N, T, H, W, C, To, Ho, Wo);
  return check_launch("maxpool3d_bwd");
}

extern "C" int avt_stem3d_wgrad_unfold(const float* dwf, float* dw, int K, int C, int KT, int R, int S, void* stream) {
  AVT_REQUIRE(dwf && dw, "stem3d_wgrad_unfold: null pointer");
  AVT_REQUIRE(K >= 1 && C >= 1 && C <= 4 && KT >= 1 && KT <= 8 && R >= 1 && S >= 1,
              "stem3d_wgrad_unfold: need C <= 4 and KT <= 8 (the 32-channel fold)");
  hipLaunchKernelGGL(stem3d_wgrad_unfold_kernel, dim3(grid_for((long long)K * C * KT * R * S)), dim3(256), 0,
                     (hipStream_t)stream, dwf, dw, K, C, KT, R, S);
  return check_launch("stem3d_wgrad_unfold");
}

extern "C" int avt_set_video_stem_dgrad(int form) {
  AVT_REQUIRE(form >= -1 && form <= 1, "set_video_stem_dgrad: form=%d (-1, 0 or 1)", form);
  avt::g_video_stem_dgrad = form;
  return AVT_OK;
}

extern "C" size_t avt_video_stem_dgrad_pack_bytes(void) { return (size_t)49 * 4096; }

extern "C" int avt_pack_video_stem_dgrad(const float* w, void* out, void* stream) {
  AVT_REQUIRE(w && out, "pack_video_stem_dgrad: null pointer");
  AVT_REQUIRE(((uintptr_t)out & 15) == 0, "pack_video_stem_dgrad: out must be 16-byte aligned");
  hipLaunchKernelGGL(pack_video_stem_dgrad_kernel, dim3(49 * 8), dim3(256), 0, (hipStream_t)stream, w, (bf16_t*)out);
  return check_launch("pack_video_stem_dgrad");
}

extern "C" int avt_video_stem_dgrad(const void* gy, const float* w, const void* wpack, float* gx, int N, int T, int H,
                                    int W, void* stream) {
  const int form = video_stem_dgrad_form();
  AVT_REQUIRE(gy && gx, "video_stem_dgrad: null pointer");
  AVT_REQUIRE(form ? wpack != nullptr : w != nullptr, "video_stem_dgrad: form %d needs %s", form,
              form ? "wpack (avt_pack_video_stem_dgrad)" : "the fp32 weight");
  AVT_REQUIRE(N >= 0 && N <= 65535 && T >= 1 && H >= 1 && W >= 1, "video_stem_dgrad: N=%d T=%d H=%d W=%d", N, T, H, W);
  AVT_REQUIRE((((uintptr_t)gy | (uintptr_t)wpack) & 15) == 0, "video_stem_dgrad: gy and wpack must be 16-byte aligned");
  const int P = (H - 1) / 2 + 1, Q = (W - 1) / 2 + 1;
  AVT_REQUIRE((long long)N * T * P * Q * 64 * 2 < (1ll << 31) && (long long)N * 3 * T * H * W * 4 < (1ll << 31),
              "video_stem_dgrad: activation tensors must stay below 2 GiB (32-bit buffer offsets)");
  if (N == 0) return AVT_OK;
  VsdArgs a{};
  a.gy = (const bf16_t*)gy;
  a.w = w;
  a.wp = (const u32x4*)wpack;
  a.gx = gx;
  a.T = T;
  a.H = H;
  a.W = W;
  a.P = P;
  a.Q = Q;
  const int order[4] = {3, 2, 1, 0};  // (odd, odd): 16 taps, then 12, 12, 9
  int nb = 0;
  for (int i = 0; i < 4; ++i) {
    const int ph = order[i] >> 1, pw = order[i] & 1;
    const long long Mc = (long long)((H - ph + 1) / 2) * ((W - pw + 1) / 2);  // 0: an empty class (H or W of 1)
    const long long blocks = form ? (Mc + 4 * kVsdPix - 1) / (4 * kVsdPix) : (Mc * T + 255) / 256;
    a.cls[i] = order[i];
    a.first[i] = nb;
    nb += (int)blocks;
  }
  a.first[4] = nb;
  if (form)
    hipLaunchKernelGGL(video_stem_dgrad_mfma_kernel, dim3(nb, N), dim3(256), kVsdLds, (hipStream_t)stream, a);
  else
    hipLaunchKernelGGL(video_stem_dgrad_direct_kernel, dim3(nb, N), dim3(256), 0, (hipStream_t)stream, a);
  return check_launch("video_stem_dgrad");
}

extern "C" size_t avt_pack3d_desc_bytes(void) { return sizeof(Pack3dDesc); }

// descs: device array of n records {const float* w; void* out; int K, C, T, pad} (avt_pack3d_desc_bytes() each):
// out[k][t*C + c] = bf16(w[k][c][t]) for every record in one launch; max_k = the largest K, max_row = the largest
// C*T (floats; <= 15360: one fp32 filter row in LDS)
extern "C" int avt_pack_conv3d_weights_batched(const void* descs, int n, int max_k, int max_row, void* stream) {
  AVT_REQUIRE(descs && n > 0 && max_k > 0, "pack_conv3d_weights_batched: bad arguments");
  AVT_REQUIRE(max_row > 0 && max_row <= 15360, "pack_conv3d_weights_batched: max_row=%d (<= 15360 floats)", max_row);
  hipLaunchKernelGGL(pack_conv3d_batched_kernel, dim3(max_k < 512 ? max_k : 512, n), dim3(256),
                     (size_t)max_row * sizeof(float), (hipStream_t)stream, (const Pack3dDesc*)descs);
  return check_launch("pack_conv3d_weights_batched");
}

extern "C" size_t avt_fold3d_desc_bytes(void) { return sizeof(Fold3dDesc); }

// descs: device array of n avt_fold3d_desc_bytes() records (include/avt.h); one launch folds them all.  max_k = the
// largest K, max_row = the largest C*KT*R*S (floats; <= 15360: one fp32 filter row in LDS)
extern "C" int avt_fold_conv3d_bn_batched(const void* descs, int n, int max_k, int max_row, void* stream) {
  AVT_REQUIRE(descs && n > 0 && max_k > 0, "fold_conv3d_bn_batched: bad arguments");
  AVT_REQUIRE(max_row > 0 && max_row <= 15360, "fold_conv3d_bn_batched: max_row=%d (<= 15360 floats)", max_row);
  hipLaunchKernelGGL(fold_conv3d_bn_batched_kernel, dim3(max_k < 512 ? max_k : 512, n), dim3(256),
                     (size_t)max_row * sizeof(float), (hipStream_t)stream, (const Fold3dDesc*)descs);
  return check_launch("fold_conv3d_bn_batched");
}

// Audio de-duplication of the tube step (train_3D.py:128-130 repeats each clip's spectrogram t
// times): the audio trunk runs once per clip; its unit vector is repeated to the (b t) rows of the
// head, and the head's gradient is summed back over the t rows (exact: everything between is linear
// in the upstream gradient for the shared forward).
extern "C" int avt_repeat_rows_f32(const float* in, float* out, int B, int rep, int C, void* stream) {
  AVT_REQUIRE(in && out && B >= 0 && rep >= 1 && C >= 1, "repeat_rows_f32: bad arguments");
  const long long n = (long long)B * rep * C;
  if (n == 0) return AVT_OK;
  hipLaunchKernelGGL(repeat_rows_kernel, dim3(grid_for(n)), dim3(256), 0, (hipStream_t)stream, in, out, B, rep, C);
  return check_launch("repeat_rows_f32");
}

extern "C" int avt_sum_rep_rows_f32(const float* in, float* out, int B, int rep, int C, void* stream) {
  AVT_REQUIRE(in && out && B >= 0 && rep >= 1 && C >= 1, "sum_rep_rows_f32: bad arguments");
  const long long n = (long long)B * C;
  if (n == 0) return AVT_OK;
  hipLaunchKernelGGL(sum_rep_rows_kernel, dim3(grid_for(n)), dim3(256), 0, (hipStream_t)stream, in, out, B, rep, C);
  return check_launch("sum_rep_rows_f32");
}
