// Train-mode BatchNorm2d (+ReLU, +residual) for the ResNet-18 trunks, NHWC bf16 activations,
// fp32 math, fp64 statistic accumulation.  Semantics of torch BatchNorm2d as used at
// models/base_models.py:39,46-49,120-121,141 (eps 1e-5, momentum 0.1): normalise with the biased
// batch variance, update running_var with the unbiased one.
//
//   fwd : the conv epilogue stores per-row-tile (sum_t, M2_t, sum_t^2/n_t) into its own slot of an fp64
//         accumulator (avt_common.h: one slot per tile or persistent block, plain stores); bn_finalize
//         merges the slots in slot order (M2 = sum M2_t + sum sum_t^2/n_t - S^2/N, Chan's formula), writes
//         scale/shift/mean/invstd and updates the running stats; bn_apply (+residual, +ReLU).
//   bwd : bn_bwd_reduce stores per-block (sum g', sum g'*xhat) (g' = g*[y>0]) into slot blockIdx of an fp64
//         accumulator -> bn_bwd_finalize (dgamma, dbeta, k1, k2) -> bn_bwd_apply:
//         g_c = gamma*invstd*(g' - k1 - xhat*k2).
//   Deterministic: no atomics; the same inputs give the same bits on every run.
//         avt_bn_relu_bwd recomputes the ReLU mask from (xc, scale, shift) instead of reading y
//         (BasicBlock.bn1, base_models.py:47-48); the stem's bn1+relu+maxpool is fused both ways
//         (avt_stem_*, below) so its full-resolution activation is never stored.
//
//   Layout of this file: the finalize kernels; then the shared pieces -- the constants' two policies (Reg8 / Mem8),
//   each formula once (bn_fwd8, relu_mask8, bn_bwd8, bn_reduce8), the row walker (walk_rows) and the reduces' block
//   epilogue (block_sums_to_slot); then the kernels, which only pick a walk (grid-stride or rows), a policy and the
//   formulas; the stem kernels (their own walk); the host launchers (reduce_deal, bn_bwd_finalize_launch,
//   with_mask_form) and the entry points.  A change to a formula or to the walk is made in one place.
#include <type_traits>

#include "avt_common.h"

namespace avt {

__device__ __forceinline__ void unpack8(const u32x4& v, float* f) {
  const unsigned* u = reinterpret_cast<const unsigned*>(&v);
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    f[2 * e] = bf2f(u[e] & 0xffff);
    f[2 * e + 1] = bf2f(u[e] >> 16);
  }
}
__device__ __forceinline__ u32x4 pack8(const float* f) {
  u32x4 v;
  v.x = pack2(f[0], f[1]);
  v.y = pack2(f[2], f[3]);
  v.z = pack2(f[4], f[5]);
  v.w = pack2(f[6], f[7]);
  return v;
}

// The slot sums of kFinCB consecutive channels [c0, c0 + kFinCB), W statistics each, in a fixed order.  A
// slot's run of E = kFinCB * W doubles is contiguous; a wave-load covers SPI = 64 / E slots (lane = (slot
// offset so, element e)), so wave w, lane (so, e) adds slots (i kFinWaves + w) SPI + so for i = 0, 1, ... in
// turn, 8 loads in flight per batch (one round trip for up to 8 * kFinWaves * SPI slots: 1024 fwd / bwd);
// the lanes' partials meet in LDS in (wave, slot offset) order.  tot[e] on return (after a barrier).
// Launch: kFinThreads threads per kFinCB channels -- many small blocks, since a finalize is latency-bound.
constexpr int kFinWaves = 16, kFinThreads = kFinWaves * 64, kFinCB = 4;
template <int W>
__device__ __forceinline__ void slot_sums(const double* __restrict__ acc, const double* __restrict__ slots, int C,
                                          int c0, long long rows, double* red, double* tot) {
  constexpr int E = kFinCB * W, SPI = 64 / E, STEP = kFinWaves * SPI;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int so = lane / E, e = lane - so * E;
  // the header's slot count, bounded by the workspace's capacity: a producer that skipped its header (or a
  // workspace handed over uninitialised) gives NaN statistics, never reads beyond the slots
  const double hn = acc[0] + acc[1];
  const bool bad = !(hn >= 0.0 && hn <= (double)bn_slot_cap(rows));
  const int n = bad ? 0 : (int)hn;
  double s = 0.0;
  if (so < SPI && c0 + e / W < C) {
    const double* base = slots + (size_t)c0 * W + e;
    const unsigned stride = (unsigned)(C * W);
    for (int k0 = w * SPI + so; k0 < n; k0 += 8 * STEP) {
      double v[8];
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        const int k = k0 + i * STEP;
        v[i] = k < n ? base[(size_t)k * stride] : 0.0;
      }
#pragma unroll
      for (int i = 0; i < 8; ++i) s += v[i];
    }
  }
  red[threadIdx.x] = s;
  __syncthreads();
  if (threadIdx.x < E) {
    double t = 0.0;
    for (int ww = 0; ww < kFinWaves; ++ww)
#pragma unroll
      for (int o = 0; o < SPI; ++o) t += red[ww * 64 + o * E + threadIdx.x];
    tot[threadIdx.x] = bad ? __builtin_nan("") : t;
  }
  __syncthreads();
}

__global__ __launch_bounds__(kFinThreads) void bn_finalize_kernel(double* __restrict__ acc, long long rows, int C,
                                                                  const float* __restrict__ gamma,
                                                                  const float* __restrict__ beta, float* running_mean,
                                                                  float* running_var, float momentum, float eps,
                                                                  float* scale, float* shift, float* save_mean,
                                                                  float* save_invstd, long long rep) {
  __shared__ double red[kFinThreads], tot[kFinCB * 3];
  const int c0 = blockIdx.x * kFinCB;
  slot_sums<3>(acc, bn_fwd_slots(acc), C, c0, rows, red, tot);
  const int c = c0 + (int)threadIdx.x;
  if (threadIdx.x >= kFinCB || c >= C) return;
  const double S = tot[threadIdx.x * 3], Q = tot[threadIdx.x * 3 + 1], R = tot[threadIdx.x * 3 + 2];
  const double n = (double)rows;
  const double mean = S / n;
  double m2 = Q + (R - S * mean);
  if (m2 < 0.0) m2 = 0.0;
  const float var = (float)(m2 / n);
  const float inv = rsqrtf(var + eps);
  const float sc = gamma[c] * inv;
  scale[c] = sc;
  shift[c] = beta[c] - (float)mean * sc;
  if (save_mean) save_mean[c] = (float)mean;
  if (save_invstd) save_invstd[c] = inv;
  if (running_mean) {
    // unbiased variance of the logical batch, in which each accumulated row occurs `rep` times
    const double nl = n * (double)rep;
    const float unb = nl > 1.0 ? (float)(m2 * (double)rep / (nl - 1.0)) : var;
    running_mean[c] = (1.f - momentum) * running_mean[c] + momentum * (float)mean;
    running_var[c] = (1.f - momentum) * running_var[c] + momentum * unb;
  }
}

// ---------------------------------------------------------------------------------------------
// The pieces every elementwise pass and every reduce below is put together from: one row walker, each formula once.

__device__ __forceinline__ u32x4 ld8(const bf16_t* p, size_t o) { return reinterpret_cast<const u32x4*>(p)[o]; }
__device__ __forceinline__ void st8(bf16_t* p, size_t o, const u32x4& v) { reinterpret_cast<u32x4*>(p)[o] = v; }

// The eight per-channel constants of a thread's channel chunk [c0, c0 + 8), by how they are reached.  Reg8: loaded
// once, into registers -- a row-walking thread keeps its chunk.  Mem8: read from memory at every use -- a grid-stride
// thread changes chunk with every vector, so there is nothing to hoist them out of (L1 hits, but each one a
// vector-memory instruction beside the 1-3 data loads).  The formulas are templates over the two, so the grid-stride
// kernels and their row-walking twins evaluate the same expression in the same order: the same bits.
struct Reg8 {
  float v[8];
  static __device__ __forceinline__ Reg8 at(const float* p, int c0) {
    Reg8 k;
#pragma unroll
    for (int e = 0; e < 8; ++e) k.v[e] = p[c0 + e];
    return k;
  }
  __device__ __forceinline__ float operator[](int e) const { return v[e]; }
  using Prod = Reg8;  // a[e] * b[e], taken once
  static __device__ __forceinline__ Prod prod(const Reg8& a, const Reg8& b) {
    Reg8 k;
#pragma unroll
    for (int e = 0; e < 8; ++e) k.v[e] = a[e] * b[e];
    return k;
  }
};
struct Mem8 {
  const float* p;
  int c0;
  static __device__ __forceinline__ Mem8 at(const float* p, int c0) { return {p, c0}; }
  __device__ __forceinline__ float operator[](int e) const { return p[c0 + e]; }
  struct Prod {  // a[e] * b[e], taken at every use
    const float *a, *b;
    int c0;
    __device__ __forceinline__ float operator[](int e) const { return a[c0 + e] * b[c0 + e]; }
  };
  static __device__ __forceinline__ Prod prod(const Mem8& a, const Mem8& b) { return {a.p, b.p, a.c0}; }
};

// Bit e of the result: bf16 element e of v is > 0 (positive and non-zero as int16) -- the ReLU
// backward's `result > 0` evaluated on the stored output.
__device__ __forceinline__ unsigned pos_bits8(const u32x4& v) {
  const unsigned* u = reinterpret_cast<const unsigned*>(&v);
  unsigned b = 0;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    b |= ((short)(u[e] & 0xffff) > 0 ? 1u : 0u) << (2 * e);
    b |= ((short)(u[e] >> 16) > 0 ? 1u : 0u) << (2 * e + 1);
  }
  return b;
}

// Forward: out = [relu]( x*scale + shift + [residual*rscale + rshift | residual] ).  res: 0 no residual, 1 + residual,
// 2 + residual*rscale + rshift.
template <class K>
__device__ __forceinline__ u32x4 bn_fwd8(const u32x4& xq, const u32x4& rq, int res, bool relu, const K& sc, const K& sh,
                                         const K& rs, const K& rh) {
  float f[8];
  unpack8(xq, f);
#pragma unroll
  for (int e = 0; e < 8; ++e) f[e] = __builtin_fmaf(f[e], sc[e], sh[e]);
  if (res) {
    float r[8];
    unpack8(rq, r);
    if (res == 2) {
#pragma unroll
      for (int e = 0; e < 8; ++e) f[e] += r[e] * rs[e] + rh[e];
    } else {
#pragma unroll
      for (int e = 0; e < 8; ++e) f[e] += r[e];
    }
  }
  if (relu) {
#pragma unroll
    for (int e = 0; e < 8; ++e) f[e] = fmaxf(f[e], 0.f);
  }
  return pack8(f);
}

// One row-vector of a backward pass as loaded: g, the pre-activation xc and whichever of the others the pass reads
// (a null pointer: not loaded, the member left as it is) -- the saved output y, the mask byte, a second BN's pre-activation.
struct BwdRow {
  u32x4 g, x, y, x2;
  unsigned bits;
};
__device__ __forceinline__ void load_bwd_row(BwdRow& v, const bf16_t* g, const bf16_t* xc, const bf16_t* y,
                                             const unsigned char* mk, const bf16_t* xc2, size_t o) {
  v.g = ld8(g, o);
  v.x = ld8(xc, o);
  if (y) v.y = ld8(y, o);
  if (xc2) v.x2 = ld8(xc2, o);
  if (mk) v.bits = mk[o];
}

// The ReLU mask of the backward pass, g' = g * [output > 0], in its four forms: none (g is g' already); the saved
// output, y > 0; recomputed from the pre-activation, relu(fma(xc, mscale, mshift)) > 0 -- the exact expression the
// forward evaluated, so the mask is identical without reading y; the bits avt_bn_apply_mask stored.
enum { kMaskNone = 0, kMaskY = 1, kMaskFma = 2, kMaskBits = 3 };
__host__ __device__ inline int mask_form(const void* y, const float* mscale) {
  return y ? kMaskY : mscale ? kMaskFma : kMaskNone;
}
template <class K = Reg8>
__device__ __forceinline__ void relu_mask8(int form, float* gg, const float* xx, const BwdRow& v, const K& ms = K{},
                                           const K& mh = K{}) {
  if (form == kMaskY) {
    float yy[8];
    unpack8(v.y, yy);
#pragma unroll
    for (int e = 0; e < 8; ++e) gg[e] = yy[e] > 0.f ? gg[e] : 0.f;
  } else if (form == kMaskFma) {
#pragma unroll
    for (int e = 0; e < 8; ++e) gg[e] = __builtin_fmaf(xx[e], ms[e], mh[e]) > 0.f ? gg[e] : 0.f;
  } else if (form == kMaskBits) {
#pragma unroll
    for (int e = 0; e < 8; ++e) gg[e] = (v.bits >> e) & 1u ? gg[e] : 0.f;
  }
}

// Backward apply: g_c = gamma*invstd*(g' - k1 - xhat*k2), xhat = (xc - mean)*invstd.
template <class K>
struct BwdK {
  K mu, is;
  typename K::Prod gi;  // gamma*invstd
  K k1, k2;
  static __device__ __forceinline__ BwdK at(const float* mean, const float* invstd, const float* gamma, const float* k1,
                                            const float* k2, int c0) {
    const K is = K::at(invstd, c0);
    return {K::at(mean, c0), is, K::prod(K::at(gamma, c0), is), K::at(k1, c0), K::at(k2, c0)};
  }
};
template <class K>
__device__ __forceinline__ u32x4 bn_bwd8(const float* gg, const float* xx, const BwdK<K>& k) {
  float v[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    const float xh = (xx[e] - k.mu[e]) * k.is[e];
    v[e] = k.gi[e] * (gg[e] - k.k1[e] - xh * k.k2[e]);
  }
  return pack8(v);
}

// Backward reduce: s1 += g' (s1 null: a second BN fed by the same g'), s2 += g' * xhat -- a product and one fused
// multiply-add, spelled out because whether the compiler fuses the plain expression depends on the code around it
// (bn_bwd_mask_reduce_kernel, below, is the kernel where it decided otherwise: it keeps its own text).
__device__ __forceinline__ void bn_reduce8(float* s1, float* s2, const float* gg, const float* xx, const Reg8& mu,
                                           const Reg8& is) {
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    if (s1) s1[e] += gg[e];
    s2[e] = __builtin_fmaf(gg[e] * (xx[e] - mu[e]), is[e], s2[e]);
  }
}

// The row walk.  Block: 256 threads; a thread owns channel chunk tid % (C/8) -- channels [c0, c0 + 8) -- and walks
// the rows r0 + k rstep (r0 = tid / (C/8), rstep = 256 / (C/8)) of its block's contiguous row range.
struct RowWalk {
  int cv, chunk, r0, rstep, c0;
  long long rows, rpb;  // the block's range: [blockIdx rpb, + rpb) of the rows
};
__device__ __forceinline__ RowWalk row_walk(int C, long long rows, long long rows_per_block) {
  RowWalk w;
  w.cv = C / 8;
  w.chunk = threadIdx.x % w.cv;
  w.r0 = threadIdx.x / w.cv;
  w.rstep = 256 / w.cv;
  w.c0 = w.chunk * 8;
  w.rows = rows;
  w.rpb = rows_per_block;
  return w;
}
// load(o) returns the operands of row-vector o (a small struct of u32x4 / a mask byte), use(v, o) consumes them.  The
// loads of U rows are issued before the first row is consumed (HBM-bound: the bytes in flight per CU set the achieved
// bandwidth); the rows left over go one at a time.
template <int U, class Row, class Load, class Use>
__device__ __forceinline__ void walk_rows(const RowWalk& w, Load load, Use use) {
  const long long rbeg = blockIdx.x * w.rpb, rend = min(w.rows, rbeg + w.rpb);
  long long r = rbeg + w.r0;
  for (; r + (U - 1) * w.rstep < rend; r += U * w.rstep) {
    const size_t o0 = (size_t)r * w.cv + w.chunk;  // row r + u rstep is 256 u vectors on (rstep cv = 256)
    Row v[U];
#pragma unroll
    for (int u = 0; u < U; ++u) load(v[u], o0 + u * 256);
#pragma unroll
    for (int u = 0; u < U; ++u) use(v[u], o0 + u * 256);
  }
  for (; U > 1 && r < rend; r += w.rstep) {  // (U = 1: the loop above took every row)
    const size_t o = (size_t)r * w.cv + w.chunk;
    Row v;
    load(v, o);
    use(v, o);
  }
}

// After a row of an unrolled iteration: the compiler may not move the next row's unpacking and arithmetic up across
// this point.  Left to itself it widens all U rows to fp32 at once for the sake of instruction-level parallelism
// these HBM-bound loops have no use for, and takes 160-240 VGPRs (two or three waves per SIMD) for it.
__device__ __forceinline__ void row_done() { __builtin_amdgcn_sched_barrier(0); }

// The block epilogue of a reduce: the threads' partials (s1, s2) meet in LDS, are summed over the rstep row groups in
// row order and go to the block's own slot of acc.  The first block records the slot count.  Every thread of the
// block calls it.
__device__ __forceinline__ void block_sums_to_slot(const RowWalk& w, int C, const float* s1, const float* s2,
                                                   double* acc) {
  __shared__ float red[2048 * 2];  // [256/(C/8)][C][2] = 4096 floats for any C
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    red[(w.r0 * C + w.c0 + e) * 2] = s1[e];
    red[(w.r0 * C + w.c0 + e) * 2 + 1] = s2[e];
  }
  __syncthreads();
  bn_write_header(acc, gridDim.x, 0);
  double* slot = bn_bwd_slots(acc, C) + (size_t)blockIdx.x * C * 2;  // this block's own slot
  for (int c = threadIdx.x; c < C; c += blockDim.x) {
    float a = 0.f, b = 0.f;
    for (int k = 0; k < w.rstep; ++k) {
      a += red[(k * C + c) * 2];
      b += red[(k * C + c) * 2 + 1];
    }
    slot[2 * c] = (double)a;
    slot[2 * c + 1] = (double)b;
  }
}

// ---------------------------------------------------------------------------------------------
// out = [relu]( x*scale + shift + [residual*rscale + rshift | residual] ), grid-stride: one thread per vector.
// The channel block of vector i is i % (C/8); POW2 (C/8 a power of two) takes it as a bit mask.
// It is the kernel of a C/8 that does not divide 256 (POW2 = false) and of AVT_BN_EW=0; every trunk shape takes the
// row-walking form below (bn_apply_rw_kernel) -- measured in profiles/bn_rowwalk_kernel_stats_b128.txt.
template <bool POW2>
__device__ __forceinline__ int chan_block(long long i, int cv) {
  return POW2 ? (int)((unsigned)i & (unsigned)(cv - 1)) : (int)(i % cv);
}

// mk (optional, with relu): the ReLU mask of out as bits, one byte per 8 channels ([rows][C/8] u8):
// the backward reads 1/16 of the bytes of out for it.
template <bool POW2>
__global__ __launch_bounds__(256) void bn_apply_kernel(const bf16_t* __restrict__ x, const float* __restrict__ scale,
                                                       const float* __restrict__ shift,
                                                       const bf16_t* __restrict__ res, const float* __restrict__ rscale,
                                                       const float* __restrict__ rshift, bf16_t* __restrict__ out,
                                                       unsigned char* __restrict__ mk, long long nvec, int C, int relu) {
  const int cv = C / 8;
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < nvec; i += (long long)gridDim.x * blockDim.x) {
    const int c0 = chan_block<POW2>(i, cv) * 8;
    const u32x4 xq = ld8(x, i);
    const u32x4 o = bn_fwd8(xq, res ? ld8(res, i) : xq, res ? (rscale ? 2 : 1) : 0, relu != 0, Mem8::at(scale, c0),
                            Mem8::at(shift, c0), Mem8::at(rscale, c0), Mem8::at(rshift, c0));
    st8(out, i, o);
    if (mk) mk[i] = (unsigned char)pos_bits8(o);
  }
}

// Per-block sums of g' and g'*xhat into slot blockIdx of the workspace, rows dealt by reduce_deal (below).  K: the
// recomputed mask's (mscale, mshift) in registers or in memory; ROW_DONE: row_done() after each consumed row.
template <class K, bool ROW_DONE>
__device__ __forceinline__ void bn_bwd_reduce_block(int form, const bf16_t* __restrict__ g, const bf16_t* __restrict__ y,
                                                    const float* __restrict__ mscale, const float* __restrict__ mshift,
                                                    const bf16_t* __restrict__ xc, const float* __restrict__ mean,
                                                    const float* __restrict__ invstd, double* __restrict__ acc,
                                                    long long rows, int C, int rows_per_block) {
  const RowWalk w = row_walk(C, rows, rows_per_block);
  const Reg8 mu = Reg8::at(mean, w.c0), is = Reg8::at(invstd, w.c0);
  const K ms = form == kMaskFma ? K::at(mscale, w.c0) : K{}, mh = form == kMaskFma ? K::at(mshift, w.c0) : K{};
  float s1[8] = {}, s2[8] = {};
  walk_rows<4, BwdRow>(
      w, [&](BwdRow& v, size_t o) { load_bwd_row(v, g, xc, form == kMaskY ? y : nullptr, nullptr, nullptr, o); },
      [&](const BwdRow& v, size_t) {
        float gg[8], xx[8];
        unpack8(v.g, gg);
        unpack8(v.x, xx);
        relu_mask8(form, gg, xx, v, ms, mh);
        bn_reduce8(s1, s2, gg, xx, mu, is);
        if (ROW_DONE) row_done();
      });
  block_sums_to_slot(w, C, s1, s2, acc);
}

// The A/B partner of bn_bwd_reduce_rw_kernel (AVT_BN_EW bit 16 off): the mask form a run-time branch, the recomputed
// mask's constants re-read for every row.
__global__ __launch_bounds__(256) void bn_bwd_reduce_kernel(const bf16_t* __restrict__ g, const bf16_t* __restrict__ y,
                                                            const float* __restrict__ mscale,
                                                            const float* __restrict__ mshift,
                                                            const bf16_t* __restrict__ xc, const float* __restrict__ mean,
                                                            const float* __restrict__ invstd, double* __restrict__ acc,
                                                            long long rows, int C, int rows_per_block) {
  bn_bwd_reduce_block<Mem8, false>(mask_form(y, mscale), g, y, mscale, mshift, xc, mean, invstd, acc, rows, C,
                                   rows_per_block);
}

// The mask form a template parameter (kMaskNone / kMaskY / kMaskFma) and the recomputed mask's (mscale, mshift) in
// registers.  Rows, slots and the order of every sum are those of bn_bwd_reduce_kernel: the slots hold the same bits.
template <int MASK>
__global__ __launch_bounds__(256) void bn_bwd_reduce_rw_kernel(const bf16_t* __restrict__ g, const bf16_t* __restrict__ y,
                                                               const float* __restrict__ mscale,
                                                               const float* __restrict__ mshift,
                                                               const bf16_t* __restrict__ xc,
                                                               const float* __restrict__ mean,
                                                               const float* __restrict__ invstd,
                                                               double* __restrict__ acc, long long rows, int C,
                                                               int rows_per_block) {
  bn_bwd_reduce_block<Reg8, true>(MASK, g, y, mscale, mshift, xc, mean, invstd, acc, rows, C, rows_per_block);
}

// dgamma/dbeta (accumulated into the gradient if non-null) and k1,k2 of channels [c0, c0 + kFinCB) from the
// slots of workspace acc (slot_sums; every thread of the block calls it)
__device__ __forceinline__ void bn_bwd_finalize_cb(double* __restrict__ acc, int C, int c0, double inv_rows,
                                                   float* dgamma, float* dbeta, float* k1, float* k2) {
  __shared__ double red[kFinThreads], tot[kFinCB * 2];
  slot_sums<2>(acc, bn_bwd_slots(acc, C), C, c0, __double2ll_rn(1.0 / inv_rows), red, tot);
  const int c = c0 + (int)threadIdx.x;
  if (threadIdx.x >= kFinCB || c >= C) return;
  const double a = tot[threadIdx.x * 2], b = tot[threadIdx.x * 2 + 1];
  if (dbeta) dbeta[c] += (float)a;
  if (dgamma) dgamma[c] += (float)b;
  k1[c] = (float)(a * inv_rows);
  k2[c] = (float)(b * inv_rows);
}

// launch: kFinThreads threads per kFinCB channels
__global__ __launch_bounds__(kFinThreads) void bn_bwd_finalize_kernel(double* __restrict__ acc, int C, double inv_rows,
                                                                      float* dgamma, float* dbeta, float* k1, float* k2) {
  bn_bwd_finalize_cb(acc, C, blockIdx.x * kFinCB, inv_rows, dgamma, dbeta, k1, k2);
}

// both BNs of a first block in one launch: blocks [0, G) the first BN's channel groups, [G, 2G) the second's
__global__ __launch_bounds__(kFinThreads) void bn_bwd_finalize2_kernel(double* __restrict__ acc, double* __restrict__ acc2,
                                                                       int C, double inv_rows, float* dgamma,
                                                                       float* dbeta, float* k1, float* k2,
                                                                       float* dgamma2, float* dbeta2, float* k1b,
                                                                       float* k2b) {
  const int G = (C + kFinCB - 1) / kFinCB;
  if ((int)blockIdx.x < G)
    bn_bwd_finalize_cb(acc, C, blockIdx.x * kFinCB, inv_rows, dgamma, dbeta, k1, k2);
  else
    bn_bwd_finalize_cb(acc2, C, (blockIdx.x - G) * kFinCB, inv_rows, dgamma2, dbeta2, k1b, k2b);
}

// g_c = gamma*invstd*(g' - k1 - xhat*k2); optionally also writes g' (masked grad) to gmask_out.  Mask: y if given, else
// (mscale, mshift) if given, else none (mask_form).
template <bool POW2>
__global__ __launch_bounds__(256) void bn_bwd_apply_kernel(const bf16_t* __restrict__ g, const bf16_t* __restrict__ y,
                                                           const float* __restrict__ mscale,
                                                           const float* __restrict__ mshift,
                                                           const bf16_t* __restrict__ xc, const float* __restrict__ mean,
                                                           const float* __restrict__ invstd,
                                                           const float* __restrict__ gamma, const float* __restrict__ k1,
                                                           const float* __restrict__ k2, bf16_t* __restrict__ gc,
                                                           bf16_t* __restrict__ gmask_out, long long nvec, int C) {
  const int cv = C / 8;
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < nvec; i += (long long)gridDim.x * blockDim.x) {
    const int c0 = chan_block<POW2>(i, cv) * 8;
    BwdRow v;
    load_bwd_row(v, g, xc, y, nullptr, nullptr, i);
    float gg[8], xx[8];
    unpack8(v.g, gg);
    unpack8(v.x, xx);
    relu_mask8(mask_form(y, mscale), gg, xx, v, Mem8::at(mscale, c0), Mem8::at(mshift, c0));
    st8(gc, i, bn_bwd8(gg, xx, BwdK<Mem8>::at(mean, invstd, gamma, k1, k2, c0)));
    if (gmask_out) st8(gmask_out, i, pack8(gg));
  }
}

// ---------------------------------------------------------------------------------------------
// Block-output BN backward from the ReLU mask bits (avt_bn_apply_mask): g' = g * bit, and -- for a
// first block -- bn2 and downsample.1 in one pass over (g, mask, xc, xc2): they share g' (the ReLU
// sits after their sum, base_models.py:64-67), so g and the mask are read once for both.
struct MaskBwdArgs {
  const bf16_t* g;
  const unsigned char* mk;  // [rows][C/8] mask bits
  const bf16_t* xc;
  const float* mean;
  const float* invstd;
  double* acc;              // [SLOTS][C][2]: (sum g', sum g' * xhat)
  const bf16_t* xc2;        // TWO: the second BN's pre-activation / statistics / accumulator
  const float* mean2;
  const float* invstd2;
  double* acc2;
  long long rows;
  int C, rows_per_block;
};

// This kernel keeps its own walk, body and three-sum epilogue.  The compiler fuses its plain `s += g' * (xc - mean) *
// invstd` into a multiply-add for some elements and not for others (none in <false>, the odd ones in <true>), and the
// slots -- with k1 / k2 / dgamma / gc behind them -- hold exactly those roundings.  On walk_rows the plain expression
// fuses differently (other bits); with the rounding spelled out per element the bits hold but <false> measured 5 %
// slower (profiles/bn_one_walker.txt, section 2).  So the text the compiler made its choice for stays as it was.
__device__ __forceinline__ void mask8(float* gg, unsigned bits) {
#pragma unroll
  for (int e = 0; e < 8; ++e) gg[e] = (bits >> e) & 1u ? gg[e] : 0.f;
}

template <bool TWO>
__global__ __launch_bounds__(256) void bn_bwd_mask_reduce_kernel(MaskBwdArgs a) {
  constexpr int NS = TWO ? 3 : 2;
  __shared__ float red[2048 * NS];  // [256/(C/8)][C][NS]
  const int C = a.C, cv = C / 8;
  const int chunk = threadIdx.x % cv, r0 = threadIdx.x / cv, rstep = 256 / cv;
  const int c0 = chunk * 8;
  float mu[8], is[8], mu2[8], is2[8], s1[8], s2[8], s3[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    mu[e] = a.mean[c0 + e];
    is[e] = a.invstd[c0 + e];
    if (TWO) {
      mu2[e] = a.mean2[c0 + e];
      is2[e] = a.invstd2[c0 + e];
    }
    s1[e] = s2[e] = s3[e] = 0.f;
  }
  const long long rbeg = (long long)blockIdx.x * a.rows_per_block;
  const long long rend = min(a.rows, rbeg + a.rows_per_block);
  auto body = [&](const u32x4& gq, unsigned bits, const u32x4& xq, const u32x4& x2q) {
    float gg[8], xx[8];
    unpack8(gq, gg);
    unpack8(xq, xx);
    mask8(gg, bits);
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      s1[e] += gg[e];
      s2[e] += gg[e] * (xx[e] - mu[e]) * is[e];
    }
    if (TWO) {
      float x2[8];
      unpack8(x2q, x2);
#pragma unroll
      for (int e = 0; e < 8; ++e) s3[e] += gg[e] * (x2[e] - mu2[e]) * is2[e];
    }
  };
  long long r = rbeg + r0;
  constexpr int U = 4;  // rows in flight per thread (HBM-bound: bytes in flight per CU)
  for (; r + (U - 1) * rstep < rend; r += U * rstep) {
    u32x4 gq[U], xq[U], x2q[U];
    unsigned bq[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const size_t o = (size_t)(r + u * rstep) * cv + chunk;
      gq[u] = reinterpret_cast<const u32x4*>(a.g)[o];
      xq[u] = reinterpret_cast<const u32x4*>(a.xc)[o];
      if (TWO) x2q[u] = reinterpret_cast<const u32x4*>(a.xc2)[o];
      bq[u] = a.mk[o];
    }
#pragma unroll
    for (int u = 0; u < U; ++u) body(gq[u], bq[u], xq[u], TWO ? x2q[u] : xq[u]);
  }
  for (; r < a.rows && r < rend; r += rstep) {
    const size_t o = (size_t)r * cv + chunk;
    const u32x4 gq = reinterpret_cast<const u32x4*>(a.g)[o];
    const u32x4 xq = reinterpret_cast<const u32x4*>(a.xc)[o];
    body(gq, a.mk[o], xq, TWO ? reinterpret_cast<const u32x4*>(a.xc2)[o] : xq);
  }
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    red[(r0 * C + c0 + e) * NS] = s1[e];
    red[(r0 * C + c0 + e) * NS + 1] = s2[e];
    if (TWO) red[(r0 * C + c0 + e) * NS + 2] = s3[e];
  }
  __syncthreads();
  bn_write_header(a.acc, gridDim.x, 0);
  if (TWO) bn_write_header(a.acc2, gridDim.x, 0);
  const size_t slot = (size_t)blockIdx.x * C * 2;  // this block's own slot
  double* s1p = bn_bwd_slots(a.acc, C) + slot;
  double* s2p = TWO ? bn_bwd_slots(a.acc2, C) + slot : nullptr;
  for (int c = threadIdx.x; c < C; c += blockDim.x) {
    float x = 0.f, y = 0.f, z = 0.f;
    for (int k = 0; k < rstep; ++k) {
      x += red[(k * C + c) * NS];
      y += red[(k * C + c) * NS + 1];
      if (TWO) z += red[(k * C + c) * NS + 2];
    }
    s1p[2 * c] = (double)x;
    s1p[2 * c + 1] = (double)y;
    if (TWO) {
      s2p[2 * c] = (double)x;
      s2p[2 * c + 1] = (double)z;
    }
  }
}

// gc = gamma*invstd*(g' - k1 - xhat*k2) (and gc2 for the second BN) from the finalized k1/k2
struct MaskApplyArgs {
  const bf16_t* g;
  const unsigned char* mk;
  const bf16_t* xc;
  const float *mean, *invstd, *gamma, *k1, *k2;
  bf16_t* gc;
  const bf16_t* xc2;
  const float *mean2, *invstd2, *gamma2, *k1b, *k2b;
  bf16_t* gc2;
  long long nvec;
  int C;
};

// row-vector o of a mask apply: k1 / k2 the constants of the first / second BN (k2 unused without TWO)
template <bool TWO, class K>
__device__ __forceinline__ void bn_bwd_mask_apply8(const MaskApplyArgs& a, const BwdRow& v, size_t o, const BwdK<K>& k1,
                                                   const BwdK<K>& k2) {
  float gg[8], xx[8];
  unpack8(v.g, gg);
  unpack8(v.x, xx);
  relu_mask8(kMaskBits, gg, xx, v);
  st8(a.gc, o, bn_bwd8(gg, xx, k1));
  if (TWO) {
    unpack8(v.x2, xx);
    st8(a.gc2, o, bn_bwd8(gg, xx, k2));
  }
}

template <bool TWO>
__global__ __launch_bounds__(256) void bn_bwd_mask_apply_kernel(MaskApplyArgs a) {
  const int cv = a.C / 8;  // a power of two dividing 256 (checked by the host)
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < a.nvec;
       i += (long long)gridDim.x * blockDim.x) {
    const int c0 = chan_block<true>(i, cv) * 8;
    BwdRow v;
    load_bwd_row(v, a.g, a.xc, nullptr, a.mk, TWO ? a.xc2 : nullptr, i);
    bn_bwd_mask_apply8<TWO>(a, v, i,
                            BwdK<Mem8>::at(a.mean, a.invstd, a.gamma, a.k1, a.k2, c0),
                            BwdK<Mem8>::at(a.mean2, a.invstd2, a.gamma2, a.k1b, a.k2b, c0));
  }
}

static int ew_grid(long long nvec) {
  long long b = (nvec + 255) / 256;
  if (b > 4096) b = 4096;
  if (b < 1) b = 1;
  return (int)b;
}

// ---------------------------------------------------------------------------------------------
// Row-walking forms of the elementwise passes (C/8 dividing 256: every trunk shape): walk_rows over the block's row
// range, the thread's 8-channel constants in registers (Reg8).  The optional operands are template parameters (no
// uniform branches in the loop).  Per element the arithmetic is the formula the grid-stride kernels above call, so
// every output bit is the same.
//
// AVT_BN_EW (read once; a performance knob, the results are the same bits): 0 = the grid-stride kernels above and
// the untemplated reduce; 1 (default) = the row-walking forms that measured faster (kBnEwDefault); any other value
// is a mask of the forms to take, for per-kernel A/B: 2 bn_apply, 4 bn_bwd_apply, 8 bn_bwd_mask_apply,
// 16 bn_bwd_reduce with its mask constants hoisted.
enum { kEwFwd = 2, kEwBwd = 4, kEwMaskBwd = 8, kEwReduce = 16 };
constexpr int kBnEwDefault = kEwFwd | kEwBwd | kEwMaskBwd | kEwReduce;
static int g_bn_ew = -1;
static bool bn_ew(int form) {
  if (g_bn_ew < 0) {
    const char* e = getenv("AVT_BN_EW");
    const int v = e ? atoi(e) : 1;
    g_bn_ew = v == 1 ? kBnEwDefault : (v > 0 ? v : 0);
  }
  return (g_bn_ew & form) != 0;
}

// The grid is sized to the chip, not to the tensor: kBnEwBlocksPerCU blocks per CU (AVT_BN_EW_BPC overrides, for
// tuning), each with a row range of whole rstep steps and at least one full unrolled iteration.
constexpr int kBnEwBlocksPerCU = 8;
struct RowDeal {
  int nblk;
  long long rpb;
};
// rows dealt to about `target` blocks: whole rstep steps, at least U of them
static RowDeal deal_rows(long long rows, int C, int target, int U) {
  const int rstep = 256 / (C / 8);
  long long rpb = (rows + target - 1) / target;
  rpb = ((rpb + rstep - 1) / rstep) * rstep;
  if (rpb < (long long)U * rstep) rpb = (long long)U * rstep;
  return {(int)((rows + rpb - 1) / rpb), rpb};
}
static RowDeal rw_deal(long long rows, int C, int U) {
  static int target = 0;  // blocks per launch: queried once
  if (target == 0) {
    int dev = 0, cus = 256;
    hipDeviceProp_t prop;
    if (hipGetDevice(&dev) == hipSuccess && hipGetDeviceProperties(&prop, dev) == hipSuccess &&
        prop.multiProcessorCount > 0)
      cus = prop.multiProcessorCount;
    const char* e = getenv("AVT_BN_EW_BPC");
    int bpc = e ? atoi(e) : kBnEwBlocksPerCU;
    if (bpc < 1) bpc = 1;
    if (bpc > 64) bpc = 64;
    target = cus * bpc;
  }
  return deal_rows(rows, C, target, U);
}
// The reduces' deal (train and eval): ~2 blocks per CU of rows -- one slot per block, and the finalize sums the slots.
static RowDeal reduce_deal(long long rows, int C) { return deal_rows(rows, C, 512, 1); }

// RES: 0 no residual, 1 + residual, 2 + residual*rscale + rshift.  MK: the ReLU mask bits (with RELU).
template <int RES, bool RELU, bool MK, int U>
__global__ __launch_bounds__(256) void bn_apply_rw_kernel(const bf16_t* __restrict__ x, const float* __restrict__ scale,
                                                          const float* __restrict__ shift,
                                                          const bf16_t* __restrict__ res,
                                                          const float* __restrict__ rscale,
                                                          const float* __restrict__ rshift, bf16_t* __restrict__ out,
                                                          unsigned char* __restrict__ mk, long long rows, int C,
                                                          long long rpb) {
  const RowWalk w = row_walk(C, rows, rpb);
  const Reg8 sc = Reg8::at(scale, w.c0), sh = Reg8::at(shift, w.c0);
  const Reg8 rs = RES == 2 ? Reg8::at(rscale, w.c0) : Reg8{}, rh = RES == 2 ? Reg8::at(rshift, w.c0) : Reg8{};
  auto one = [&](const u32x4& xq, const u32x4& rq, size_t o) {
    const u32x4 q = bn_fwd8(xq, rq, RES, RELU, sc, sh, rs, rh);
    st8(out, o, q);
    if (MK) mk[o] = (unsigned char)pos_bits8(q);
    row_done();
  };
  // walk_rows' loop written out, with x and the residual in two arrays: as one struct per row behind the walker's
  // callables the <1, relu, mask> and <2, relu, *> forms took 1-4 VGPRs more (79 -> 81: a wave per SIMD)
  const long long rbeg = blockIdx.x * rpb, rend = min(rows, rbeg + rpb);
  long long r = rbeg + w.r0;
  for (; r + (U - 1) * w.rstep < rend; r += U * w.rstep) {
    const size_t o0 = (size_t)r * w.cv + w.chunk;  // row r + u rstep is 256 u vectors on (rstep cv = 256)
    u32x4 xq[U], rq[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      xq[u] = ld8(x, o0 + u * 256);
      if (RES) rq[u] = ld8(res, o0 + u * 256);
    }
#pragma unroll
    for (int u = 0; u < U; ++u) one(xq[u], RES ? rq[u] : xq[u], o0 + u * 256);
  }
  for (; r < rend; r += w.rstep) {
    const size_t o = (size_t)r * w.cv + w.chunk;
    const u32x4 xq = ld8(x, o);
    one(xq, RES ? ld8(res, o) : xq, o);
  }
}

template <int RES, bool RELU, bool MK>
static void bn_apply_rw_launch(const bf16_t* x, const float* scale, const float* shift, const bf16_t* res,
                               const float* rscale, const float* rshift, bf16_t* out, unsigned char* mk,
                               long long rows, int C, hipStream_t st) {
  constexpr int U = 4;
  const RowDeal d = rw_deal(rows, C, U);
  hipLaunchKernelGGL((bn_apply_rw_kernel<RES, RELU, MK, U>), dim3(d.nblk), dim3(256), 0, st, x, scale, shift, res,
                     rscale, rshift, out, mk, rows, C, d.rpb);
}

// the instantiations avt_bn_apply (MK = false: relu 0 / 1) and avt_bn_apply_mask (MK = true: always ReLU) reach
template <bool MK>
static void bn_apply_rw_dispatch(const bf16_t* x, const float* scale, const float* shift, const bf16_t* res,
                                 const float* rscale, const float* rshift, bf16_t* out, unsigned char* mk,
                                 long long rows, int C, int relu, hipStream_t st) {
#define AVT_FWD_RW(RES)                                                                                     \
  do {                                                                                                      \
    if (MK || relu)                                                                                         \
      bn_apply_rw_launch<RES, true, MK>(x, scale, shift, res, rscale, rshift, out, mk, rows, C, st);        \
    else                                                                                                    \
      bn_apply_rw_launch<RES, false, false>(x, scale, shift, res, rscale, rshift, out, mk, rows, C, st);    \
  } while (0)
  if (!res)
    AVT_FWD_RW(0);
  else if (!rscale)
    AVT_FWD_RW(1);
  else
    AVT_FWD_RW(2);
#undef AVT_FWD_RW
}

// The launchers' one mask-form dispatch: f(std::integral_constant<int, form>) of mask_form(y, mscale).
template <class F>
static void with_mask_form(const void* y, const float* mscale, F f) {
  switch (mask_form(y, mscale)) {
    case kMaskY: return f(std::integral_constant<int, kMaskY>{});
    case kMaskFma: return f(std::integral_constant<int, kMaskFma>{});
    default: return f(std::integral_constant<int, kMaskNone>{});
  }
}

// MASK: kMaskNone (g is g'), kMaskY, kMaskFma.  GM: also writes g' to gmask_out.
template <int MASK, bool GM, int U>
__global__ __launch_bounds__(256) void bn_bwd_apply_rw_kernel(
    const bf16_t* __restrict__ g, const bf16_t* __restrict__ y, const float* __restrict__ mscale,
    const float* __restrict__ mshift, const bf16_t* __restrict__ xc, const float* __restrict__ mean,
    const float* __restrict__ invstd, const float* __restrict__ gamma, const float* __restrict__ k1,
    const float* __restrict__ k2, bf16_t* __restrict__ gc, bf16_t* __restrict__ gmask_out, long long rows, int C,
    long long rpb) {
  const RowWalk w = row_walk(C, rows, rpb);
  const BwdK<Reg8> k = BwdK<Reg8>::at(mean, invstd, gamma, k1, k2, w.c0);
  const Reg8 ms = MASK == kMaskFma ? Reg8::at(mscale, w.c0) : Reg8{}, mh = MASK == kMaskFma ? Reg8::at(mshift, w.c0) : Reg8{};
  walk_rows<U, BwdRow>(
      w, [&](BwdRow& v, size_t o) { load_bwd_row(v, g, xc, MASK == kMaskY ? y : nullptr, nullptr, nullptr, o); },
      [&](const BwdRow& v, size_t o) {
        float gg[8], xx[8];
        unpack8(v.g, gg);
        unpack8(v.x, xx);
        relu_mask8(MASK, gg, xx, v, ms, mh);
        st8(gc, o, bn_bwd8(gg, xx, k));
        if (GM) st8(gmask_out, o, pack8(gg));
        row_done();
      });
}

// the form of bn_bwd_apply_kernel<true>'s arguments; avt_bn_relu_bwd (kMaskFma) has no gmask_out
static void bn_bwd_apply_rw_launch(const bf16_t* g, const bf16_t* y, const float* mscale, const float* mshift,
                                   const bf16_t* xc, const float* mean, const float* invstd, const float* gamma,
                                   const float* k1, const float* k2, bf16_t* gc, bf16_t* gmask_out, long long rows,
                                   int C, hipStream_t st) {
  constexpr int U = 4;
  const RowDeal d = rw_deal(rows, C, U);
  with_mask_form(y, mscale, [&](auto m) {
    constexpr int MASK = decltype(m)::value;
    auto launch = [&](auto gm) {
      hipLaunchKernelGGL((bn_bwd_apply_rw_kernel<MASK, decltype(gm)::value, U>), dim3(d.nblk), dim3(256), 0, st, g, y,
                         mscale, mshift, xc, mean, invstd, gamma, k1, k2, gc, gmask_out, rows, C, d.rpb);
    };
    if constexpr (MASK != kMaskFma)
      if (gmask_out) return launch(std::true_type{});
    launch(std::false_type{});
  });
}

// bn_bwd_mask_apply_kernel's row-walking form (MaskApplyArgs::nvec = rows * C/8)
template <bool TWO, int U>
__global__ __launch_bounds__(256) void bn_bwd_mask_apply_rw_kernel(MaskApplyArgs a, long long rows, long long rpb) {
  const RowWalk w = row_walk(a.C, rows, rpb);
  const BwdK<Reg8> k1 = BwdK<Reg8>::at(a.mean, a.invstd, a.gamma, a.k1, a.k2, w.c0);
  const BwdK<Reg8> k2 = TWO ? BwdK<Reg8>::at(a.mean2, a.invstd2, a.gamma2, a.k1b, a.k2b, w.c0) : BwdK<Reg8>{};
  walk_rows<U, BwdRow>(
      w, [&](BwdRow& v, size_t o) { load_bwd_row(v, a.g, a.xc, nullptr, a.mk, TWO ? a.xc2 : nullptr, o); },
      [&](const BwdRow& v, size_t o) {
        bn_bwd_mask_apply8<TWO>(a, v, o, k1, k2);
        row_done();
      });
}

template <bool TWO>
static void bn_bwd_mask_apply_rw_launch(const MaskApplyArgs& p, long long rows, hipStream_t st) {
  constexpr int U = TWO ? 2 : 4;  // (TWO holds 80 constants: two rows in flight keep it at four waves per SIMD)
  const RowDeal d = rw_deal(rows, p.C, U);
  hipLaunchKernelGGL((bn_bwd_mask_apply_rw_kernel<TWO, U>), dim3(d.nblk), dim3(256), 0, st, p, rows, d.rpb);
}

// ---------------------------------------------------------------------------------------------
// Stem: bn1 -> relu -> MaxPool2d(3,2,1) (models/base_models.py:200-203) without materialising the
// full-resolution activation h0 = relu(bn(c0)), the largest tensor of either trunk.
//   fwd : one thread per (pooled pixel, 8 channels) evaluates h0 on its 3x3 window exactly as
//         bn_apply would (fma, relu, bf16 round), keeps the first max, and writes the pooled value,
//         the window argmax and carg = c0 at the argmax (the only pre-activations the backward's
//         reduction needs).
//   bwd : g'(h,w) = [h0(h,w) > 0] * sum of gy over the windows whose argmax is (h,w).  Its two
//         BN reductions (sum g', sum g'*xhat) are taken over the pooled grid from (gy, carg) --
//         a position picked by several windows contributes once per window, which sums to the
//         same total -- and the apply pass gathers g' per input pixel like maxpool3s2_bwd.
// One block per output row (n, p) [fwd] / input row (n, h) [bwd]; the block's threads stride over
// that row's (column, 8-channel block) items; cv = C/8 = 1 << cvs.
__global__ __launch_bounds__(256) void stem_bn_relu_maxpool_fwd_kernel(
    const bf16_t* __restrict__ c, const float* __restrict__ scale, const float* __restrict__ shift,
    bf16_t* __restrict__ y, unsigned char* __restrict__ idx, bf16_t* __restrict__ carg, int H, int W, int C, int cvs,
    int P, int Q) {
  const int row = blockIdx.x;  // n * P + p
  const int n = row / P, p = row - n * P;
  const int cv = 1 << cvs;
  const bf16_t* cimg = c + (size_t)n * H * W * C;
  // window rows 2p-1+r, r = 0..2 (validity is block-uniform); loads use clamped coordinates and
  // out-of-image taps are masked, so all nine 16-B loads of a thread issue together
  bool rok[3];
  int hh[3];
#pragma unroll
  for (int r = 0; r < 3; ++r) {
    const int h = p * 2 - 1 + r;
    rok[r] = h >= 0 && h < H;
    hh[r] = min(max(h, 0), H - 1);
  }
  for (int t = threadIdx.x; t < Q * cv; t += 256) {
    const int q = t >> cvs, c8 = t & (cv - 1);
    float sc[8], sh[8], best[8], bc[8];
    int bi[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      sc[e] = scale[c8 * 8 + e];
      sh[e] = shift[c8 * 8 + e];
      best[e] = -INFINITY;
      bc[e] = 0.f;
      bi[e] = 0;
    }
    u32x4 v[9];
    bool ok[9];
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
      for (int s2 = 0; s2 < 3; ++s2) {
        const int w = q * 2 - 1 + s2;
        ok[r * 3 + s2] = rok[r] && w >= 0 && w < W;
        const int wc = min(max(w, 0), W - 1);
        v[r * 3 + s2] = *reinterpret_cast<const u32x4*>(cimg + ((size_t)hh[r] * W + wc) * C + c8 * 8);
      }
#pragma unroll
    for (int k = 0; k < 9; ++k) {
      if (!ok[k]) continue;
      float xv[8];
      unpack8(v[k], xv);
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const float f = bf2f(f2bf(fmaxf(__builtin_fmaf(xv[e], sc[e], sh[e]), 0.f)));
        if (f > best[e] || f != f) {
          best[e] = f;
          bc[e] = xv[e];
          bi[e] = k;
        }
      }
    }
    const size_t off = ((size_t)row * Q + q) * C + c8 * 8;
    *reinterpret_cast<u32x4*>(y + off) = pack8(best);
    *reinterpret_cast<u32x4*>(carg + off) = pack8(bc);
    unsigned long long ib = 0;
#pragma unroll
    for (int e = 0; e < 8; ++e) ib |= (unsigned long long)bi[e] << (8 * e);
    *reinterpret_cast<unsigned long long*>(idx + off) = ib;
  }
}

// LDS capacity for the two pooled rows a bwd block reads: 2 x Q x C x (2 B grad + 1 B argmax)
constexpr int kStemLdsBytes = 48 * 1024;

// One block per PAIR of input rows (2p, 2p+1) of image n: the windows covering them are pooled rows p
// (row 2p: window row kh = 1; row 2p+1: kh = 2) and p+1 (row 2p+1: kh = 0), so the block stages those two
// pooled rows of gy and argmax into LDS once for both input rows (a row per block staged ~1.5 pooled rows
// per input row) and has twice the items in flight.  For input pixel (h, w) the candidate windows are
// (p_h, q) with q = w/2 (kw = 1 if w even, 2 if odd) and, for odd w, q+1 (kw = 0); g' = [h0 > 0] * the
// sum of gy over the candidates whose argmax is (h, w); gc = gamma*invstd*(g' - k1 - xhat*k2).
// EVAL: the running-statistics rule gc = gamma*invstd*g' (mean / k1 / k2 are not read).
constexpr int kStemBwdThreads = 512;
template <bool EVAL>
__global__ __launch_bounds__(kStemBwdThreads) void stem_maxpool_bn_bwd_apply_kernel(
    const bf16_t* __restrict__ gy, const unsigned char* __restrict__ idx, const bf16_t* __restrict__ c,
    const float* __restrict__ scale, const float* __restrict__ shift, const float* __restrict__ mean,
    const float* __restrict__ invstd, const float* __restrict__ gamma, const float* __restrict__ k1,
    const float* __restrict__ k2, bf16_t* __restrict__ gc, int H, int W, int C, int cvs, int P, int Q) {
  extern __shared__ __attribute__((aligned(16))) char lds[];  // 6*Q*C bytes (dynamic)
  const int hp = (H + 1) >> 1;
  const int n = blockIdx.x / hp, p = blockIdx.x - n * hp;
  const int cv = 1 << cvs;
  const bool two_rows = 2 * p + 1 < H;
  const bool p_next = p + 1 < P;
  const int rowg = Q * C * 2, rowi = Q * C;  // bytes of one pooled row of gy / argmax
  bf16_t* lg = reinterpret_cast<bf16_t*>(lds);
  unsigned char* li = reinterpret_cast<unsigned char*>(lds + 2 * rowg);
  const int items_row = W * cv, items = (two_rows ? 2 : 1) * items_row;
  // the pre-activations of this thread's items first: independent of the staged rows, their HBM latency
  // overlaps the staging and its barrier
  constexpr int kItems = 6;
  u32x4 cx[kItems];
  const size_t img_row0 = (size_t)n * H + 2 * p;  // input row 2p of image n
  // item t -> (input row 2p + r, pixel w, the thread's channel chunk): per row the even pixels first, then the
  // odd ones, so that a wave's items share their candidate-window pattern (even h / w: one window row / column,
  // odd: two) and the absent candidates are skipped by wave-uniform branches
  const int cw = threadIdx.x & (cv - 1), we_items = ((W + 1) >> 1) * cv;
  auto item_pix = [&](int t, int& r, int& w) {
    r = t >= items_row ? 1 : 0;
    const int tw = t - r * items_row;
    w = tw < we_items ? 2 * (tw >> cvs) : 2 * ((tw - we_items) >> cvs) + 1;
  };
#pragma unroll
  for (int j = 0; j < kItems; ++j) {
    const int t = threadIdx.x + kStemBwdThreads * j;
    if (t < items) {
      int r, w;
      item_pix(t, r, w);
      cx[j] = *reinterpret_cast<const u32x4*>(c + ((img_row0 + r) * W + w) * C + cw * 8);
    }
  }
  // the thread's 8 channels are the same for all its items (kStemBwdThreads is a multiple of C / 8): their
  // per-channel constants are loaded once, not per item (7 x 8 scalar loads per item were the kernel's
  // vector-memory instruction stream)
  const int c8 = cw;
  float k_sc[8], k_sh[8], k_mu[8], k_is[8], k_k1[8], k_k2[8], k_gi[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    const int ch = c8 * 8 + e;
    k_sc[e] = scale[ch];
    k_sh[e] = shift[ch];
    k_is[e] = invstd[ch];
    k_mu[e] = EVAL ? 0.f : mean[ch];
    k_k1[e] = EVAL ? 0.f : k1[ch];
    k_k2[e] = EVAL ? 0.f : k2[ch];
    k_gi[e] = gamma[ch] * k_is[e];
  }
  // stage the (<= 2) pooled rows of gy and argmax: every load issued before any LDS store
  const int ng = rowg / 16, ni = rowi / 16, nrows = p_next ? 2 : 1, nst = nrows * (ng + ni);
  constexpr int kStage = 4;
  u32x4 sv[kStage];
  const u32x4* sg = reinterpret_cast<const u32x4*>(gy + ((size_t)n * P + p) * Q * C);
  const u32x4* si = reinterpret_cast<const u32x4*>(idx + ((size_t)n * P + p) * Q * C);
  // rounds of kStage loads per thread (one round up to W = 168 at C = 64; wider rows take more, up to the LDS bound)
  for (int t0 = 0; t0 < nst; t0 += kStage * kStemBwdThreads) {
#pragma unroll
    for (int j = 0; j < kStage; ++j) {
      const int t = t0 + threadIdx.x + kStemBwdThreads * j;
      if (t < nst) sv[j] = t < nrows * ng ? sg[t] : si[t - nrows * ng];  // consecutive pooled rows are contiguous
    }
#pragma unroll
    for (int j = 0; j < kStage; ++j) {
      const int t = t0 + threadIdx.x + kStemBwdThreads * j;
      if (t < nst) {
        char* dst = t < nrows * ng ? lds + (size_t)t * 16 : lds + 2 * rowg + (size_t)(t - nrows * ng) * 16;
        *reinterpret_cast<u32x4*>(dst) = sv[j];
      }
    }
  }
  __syncthreads();
#pragma unroll
  for (int j = 0; j < kItems; ++j) {
    const int t = threadIdx.x + kStemBwdThreads * j;
    if (t >= items) break;
    int r, w;
    item_pix(t, r, w);
    // window row of (2p + r) in pooled row p: kh0 = 1 + r; in pooled row p + 1 (odd rows only): kh0 - 2;
    // column: q0 = w / 2 at kw0 (1 for even w, 2 for odd) and, odd w only, q0 + 1 at kw0 - 2
    const int kh0 = 1 + r, q0 = w >> 1, kw0 = (w & 1) + 1;
    const bool p_two = r == 1 && p_next, q_two = (w & 1) && q0 + 1 < Q;
    float gg[8], xx[8], o[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) gg[e] = 0.f;
    // g' += gy of a candidate window whose argmax is (h, w), in the order (p, q0), (p, q0+1), (p+1, q0), (p+1, q0+1)
    auto cand = [&](int lrow, int q, int pos) {
      const int el = lrow * Q * C + q * C + c8 * 8;
      const unsigned long long iv = *reinterpret_cast<const unsigned long long*>(li + el);
      float f[8];
      unpack8(*reinterpret_cast<const u32x4*>(lg + el), f);
#pragma unroll
      for (int e = 0; e < 8; ++e) gg[e] += ((int)((iv >> (8 * e)) & 0xff) == pos) ? f[e] : 0.f;
    };
    cand(0, q0, kh0 * 3 + kw0);
    if (q_two) cand(0, q0 + 1, kh0 * 3 + kw0 - 2);
    if (p_two) {
      cand(1, q0, (kh0 - 2) * 3 + kw0);
      if (q_two) cand(1, q0 + 1, (kh0 - 2) * 3 + kw0 - 2);
    }
    const size_t xo = ((img_row0 + r) * W + w) * C + c8 * 8;
    unpack8(cx[j], xx);
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      gg[e] = __builtin_fmaf(xx[e], k_sc[e], k_sh[e]) > 0.f ? gg[e] : 0.f;
      if (EVAL) {
        o[e] = __builtin_fmaf(k_gi[e], gg[e], 0.f);  // (+ 0: a pixel with g' = 0 gets +0 whatever gamma's sign)
      } else {
        const float xh = (xx[e] - k_mu[e]) * k_is[e];
        o[e] = k_gi[e] * (gg[e] - k_k1[e] - xh * k_k2[e]);
      }
    }
    *reinterpret_cast<u32x4*>(gc + xo) = pack8(o);
  }
}

static void bn_bwd_reduce_launch(const bf16_t* g, const bf16_t* y, const float* mscale, const float* mshift,
                                 const bf16_t* xc, const float* mean, const float* invstd, double* acc, long long rows,
                                 int C, hipStream_t st) {
  const RowDeal d = reduce_deal(rows, C);
  if (!bn_ew(kEwReduce))
    hipLaunchKernelGGL(bn_bwd_reduce_kernel, dim3(d.nblk), dim3(256), 0, st, g, y, mscale, mshift, xc, mean, invstd,
                       acc, rows, C, (int)d.rpb);
  else
    with_mask_form(y, mscale, [&](auto m) {
      hipLaunchKernelGGL(bn_bwd_reduce_rw_kernel<decltype(m)::value>, dim3(d.nblk), dim3(256), 0, st, g, y, mscale,
                         mshift, xc, mean, invstd, acc, rows, C, (int)d.rpb);
    });
}

// k1 / k2 of a backward workspace: 2C floats behind the header (avt_common.h)
static float* bn_k1(double* acc) { return (float*)(acc + kBnHdr); }

// The finalize of one backward workspace, or of two in one launch (acc2: a first block's second BN): dgamma / dbeta
// are added into the gradients, k1 / k2 left in the workspace.  diag: under AVT_DIAG_SKIP bit 64 it is launched once
// more, under bit 2 not at all (timing only).
static void bn_bwd_finalize_launch(hipStream_t st, int C, double inv_rows, bool diag, double* acc, float* dgamma,
                                   float* dbeta, double* acc2 = nullptr, float* dgamma2 = nullptr,
                                   float* dbeta2 = nullptr) {
  const int G = (C + kFinCB - 1) / kFinCB;
  auto launch = [&] {
    if (acc2)
      hipLaunchKernelGGL(bn_bwd_finalize2_kernel, dim3(2 * G), dim3(kFinThreads), 0, st, acc, acc2, C, inv_rows, dgamma,
                         dbeta, bn_k1(acc), bn_k1(acc) + C, dgamma2, dbeta2, bn_k1(acc2), bn_k1(acc2) + C);
    else
      hipLaunchKernelGGL(bn_bwd_finalize_kernel, dim3(G), dim3(kFinThreads), 0, st, acc, C, inv_rows, dgamma, dbeta,
                         bn_k1(acc), bn_k1(acc) + C);
  };
  if (diag && diag_skip(64, st)) launch();
  if (!diag || !diag_skip(2, st)) launch();
}

// ---------------------------------------------------------------------------------------------
// Eval-mode (running-statistics) BatchNorm backward.  With fixed statistics BN is a per-channel affine map, so the
// mean terms of the train-mode rule vanish and one pass does everything: g' = g * mask, gc = gamma*invstd*g' (and
// gc2 of a second BN fed by the same g': a first block's bn2 + downsample.1), and -- only for a BN whose dgamma or
// dbeta is wanted -- the block's (sum g', sum g'*xhat) into its own slot of the fixed-order workspace, xhat =
// (xc - running_mean)*invstd.  Rows are dealt to blocks and threads as in the train-mode reduces (one row at a time).
struct EvalBwdArgs {
  const bf16_t* g;
  const bf16_t* y;      // mask y > 0, or
  const float* mscale;  // mask fma(xc, mscale, mshift) > 0 (xc of the first BN), or none
  const float* mshift;
  const unsigned char* mk;  // BITS: mask = the [rows][C/8] bits of avt_bn_apply_mask
  bf16_t* gmask_out;    // optional g'
  const bf16_t* xc[2];
  const float* mean[2];
  const float* invstd[2];
  const float* gamma[2];
  bf16_t* gc[2];
  double* acc[2];       // NULL: no parameter gradient of that BN, nothing is reduced
  long long rows;
  int C, rows_per_block;
};

template <bool TWO, bool BITS>
__global__ __launch_bounds__(256) void bn_eval_bwd_kernel(EvalBwdArgs a) {
  constexpr int NB = TWO ? 2 : 1;
  const RowWalk w = row_walk(a.C, a.rows, a.rows_per_block);
  const int form = BITS ? kMaskBits : mask_form(a.y, a.mscale);
  Reg8 mu[NB], is[NB], gi[NB];
  float s1[8] = {}, s2[NB][8] = {};
#pragma unroll
  for (int b = 0; b < NB; ++b) {
    mu[b] = Reg8::at(a.mean[b], w.c0);
    is[b] = Reg8::at(a.invstd[b], w.c0);
    gi[b] = Reg8::at(a.gamma[b], w.c0);
#pragma unroll
    for (int e = 0; e < 8; ++e) gi[b].v[e] *= is[b][e];
  }
  // target b of row-vector o: its share of the sums, and gc = gamma*invstd*g'
  auto target = [&](int b, const float* gg, const float* xx, size_t o) {
    float v[8];
    bn_reduce8(b ? nullptr : s1, s2[b], gg, xx, mu[b], is[b]);
#pragma unroll
    for (int e = 0; e < 8; ++e) v[e] = gi[b][e] * gg[e];
    st8(a.gc[b], o, pack8(v));
  };
  walk_rows<1, BwdRow>(
      w,
      [&](BwdRow& v, size_t o) { load_bwd_row(v, a.g, a.xc[0], form == kMaskY ? a.y : nullptr, BITS ? a.mk : nullptr, nullptr, o); },
      [&](const BwdRow& v, size_t o) {
        float gg[8], xx[8];
        unpack8(v.g, gg);
        unpack8(v.x, xx);
        relu_mask8(form, gg, xx, v, Mem8::at(a.mscale, w.c0), Mem8::at(a.mshift, w.c0));
        target(0, gg, xx, o);
        if (a.gmask_out) st8(a.gmask_out, o, pack8(gg));
        if (TWO) {
          unpack8(ld8(a.xc[NB - 1], o), xx);  // (read here, after the first BN's store: one row's operands at a time)
          target(NB - 1, gg, xx, o);
        }
      });
#pragma unroll
  for (int b = 0; b < NB; ++b) {
    if (!a.acc[b]) continue;  // (uniform over the block)
    __syncthreads();          // (the LDS of the other target's sums has been read)
    block_sums_to_slot(w, a.C, s1, s2[b], a.acc[b]);
  }
}

}  // namespace avt

using namespace avt;

// The launches of avt_bn_eval_bwd / avt_bn_eval_bwd_mask: a (mask fields set by the caller) gets the targets and the
// reduces' row deal; the pass, then a finalize per target whose dgamma or dbeta is wanted.
static int bn_eval_bwd_launch(EvalBwdArgs& a, const avt_bn_bwd_target* t1, const avt_bn_bwd_target* t2, long long rows,
                              int C, void* stream, const char* who) {
  AVT_REQUIRE(C % 8 == 0 && C <= 2048 && 256 % (C / 8) == 0, "%s: C=%d unsupported", who, C);
  AVT_REQUIRE(rows > 0, "%s: empty input", who);
  const avt_bn_bwd_target* ts[2] = {t1, t2};
  for (int k = 0; k < (t2 ? 2 : 1); ++k) {
    const avt_bn_bwd_target* t = ts[k];
    AVT_REQUIRE(t->xc && t->mean && t->invstd && t->gamma && t->gc, "%s: null target pointer", who);
    const bool wants = t->dgamma || t->dbeta;
    AVT_REQUIRE(!wants || (t->workspace && ((uintptr_t)t->workspace & 7) == 0),
                "%s: dgamma/dbeta need an 8-byte aligned workspace", who);
    a.xc[k] = (const bf16_t*)t->xc;
    a.mean[k] = t->mean;
    a.invstd[k] = t->invstd;
    a.gamma[k] = t->gamma;
    a.gc[k] = (bf16_t*)t->gc;
    a.acc[k] = wants ? (double*)t->workspace : nullptr;
  }
  a.rows = rows;
  a.C = C;
  const RowDeal d = reduce_deal(rows, C);
  a.rows_per_block = (int)d.rpb;
  hipStream_t st = (hipStream_t)stream;
  auto launch = [&](auto two, auto bits) {
    hipLaunchKernelGGL((bn_eval_bwd_kernel<decltype(two)::value, decltype(bits)::value>), dim3(d.nblk), dim3(256), 0, st,
                       a);
  };
  if (a.mk) {
    if (t2) launch(std::true_type{}, std::true_type{}); else launch(std::false_type{}, std::true_type{});
  } else {
    if (t2) launch(std::true_type{}, std::false_type{}); else launch(std::false_type{}, std::false_type{});
  }
  for (int k = 0; k < (t2 ? 2 : 1); ++k)  // (k1 / k2, the train-mode rule's means: written, not used here)
    if (a.acc[k]) bn_bwd_finalize_launch(st, C, 1.0 / (double)rows, false, a.acc[k], ts[k]->dgamma, ts[k]->dbeta);
  return check_launch(who);
}

// Eval-mode BatchNorm backward (see bn_eval_bwd_kernel).  t1 (and t2, sharing g') as avt_bn_bwd_mask's targets with
// mean = running_mean and invstd = rsqrt(running_var + eps); a target's workspace is read only when its dgamma or
// dbeta is non-NULL.  Mask: y (y > 0) if given, else (mscale, mshift) on t1's xc if given, else none.
extern "C" int avt_bn_eval_bwd(const void* g, const void* y, const float* mscale, const float* mshift,
                               const avt_bn_bwd_target* t1, const avt_bn_bwd_target* t2, void* gmask_out,
                               long long rows, int C, void* stream) {
  AVT_REQUIRE(g && t1, "bn_eval_bwd: null pointer");
  AVT_REQUIRE((mscale == nullptr) == (mshift == nullptr), "bn_eval_bwd: mscale/mshift must be both set or both null");
  EvalBwdArgs a{};
  a.g = (const bf16_t*)g;
  a.y = (const bf16_t*)y;
  a.mscale = y ? nullptr : mscale;
  a.mshift = y ? nullptr : mshift;
  a.gmask_out = (bf16_t*)gmask_out;
  return bn_eval_bwd_launch(a, t1, t2, rows, C, stream, "bn_eval_bwd");
}

// avt_bn_eval_bwd with the mask read from the bits of avt_bn_apply_mask (a 2-D block output: 1/16 of the bytes of
// the stored output).  The same kernel body, row dealing and slot order: where the bits are [out > 0] the results are
// those of avt_bn_eval_bwd(y = out) bit for bit.
extern "C" int avt_bn_eval_bwd_mask(const void* g, const void* mask, const avt_bn_bwd_target* t1,
                                    const avt_bn_bwd_target* t2, long long rows, int C, void* stream) {
  AVT_REQUIRE(g && mask && t1, "bn_eval_bwd_mask: null pointer");
  EvalBwdArgs a{};
  a.g = (const bf16_t*)g;
  a.mk = (const unsigned char*)mask;
  return bn_eval_bwd_launch(a, t1, t2, rows, C, stream, "bn_eval_bwd_mask");
}

extern "C" size_t avt_bn_acc_doubles(long long rows, int C) {
  return rows < 0 || C <= 0 ? 0 : (size_t)kBnHdr + (size_t)bn_slot_cap(rows) * C * 3;
}

extern "C" int avt_bn_finalize(double* acc, long long rows, int C, const float* gamma, const float* beta,
                               float* running_mean, float* running_var, float momentum, float eps, float* scale,
                               float* shift, float* save_mean, float* save_invstd, void* stream) {
  AVT_REQUIRE(acc && gamma && beta && scale && shift, "bn_finalize: null pointer");
  AVT_REQUIRE(rows > 0 && C > 0, "bn_finalize: empty input");
  hipStream_t st = (hipStream_t)stream;
  if (diag_skip(1, st)) return AVT_OK;
  for (int rep = diag_skip(32, st) ? 2 : 1; rep > 0; --rep)  // (AVT_DIAG bit 32: each launched twice, timing only)
    hipLaunchKernelGGL(bn_finalize_kernel, dim3((C + kFinCB - 1) / kFinCB), dim3(kFinThreads), 0, st, acc, rows, C,
                       gamma, beta, running_mean, running_var, momentum, eps, scale, shift, save_mean, save_invstd, 1LL);
  return check_launch("bn_finalize");
}

// As avt_bn_finalize for a logical batch in which every accumulated row occurs `rep` times (the
// tube step's t-fold repeated spectrogram, train_3D.py:128-130, run once per distinct clip):
// mean and biased variance are those of the distinct rows; the running variance gets the
// unbiased factor of the rows*rep logical rows, exactly as BatchNorm2d over the repeated batch.
extern "C" int avt_bn_finalize_rep(double* acc, long long rows, long long rep, int C, const float* gamma,
                                   const float* beta, float* running_mean, float* running_var, float momentum,
                                   float eps, float* scale, float* shift, float* save_mean, float* save_invstd,
                                   void* stream) {
  AVT_REQUIRE(acc && gamma && beta && scale && shift, "bn_finalize_rep: null pointer");
  AVT_REQUIRE(rows > 0 && C > 0 && rep >= 1, "bn_finalize_rep: empty input");
  if (!diag_skip(1, (hipStream_t)stream)) hipLaunchKernelGGL(bn_finalize_kernel, dim3((C + kFinCB - 1) / kFinCB), dim3(kFinThreads), 0, (hipStream_t)stream, acc, rows, C, gamma,
                     beta, running_mean, running_var, momentum, eps, scale, shift, save_mean, save_invstd, rep);
  return check_launch("bn_finalize_rep");
}

extern "C" int avt_bn_apply(const void* x, const float* scale, const float* shift, const void* residual,
                            const float* rscale, const float* rshift, void* out, long long rows, int C, int relu,
                            void* stream) {
  AVT_REQUIRE(x && scale && shift && out, "bn_apply: null pointer");
  AVT_REQUIRE(C % 8 == 0, "bn_apply: C=%d must be a multiple of 8", C);
  AVT_REQUIRE((rscale == nullptr) == (rshift == nullptr), "bn_apply: rscale/rshift must be both set or both null");
  const long long nvec = rows * C / 8;
  if (nvec == 0 || diag_skip(16, (hipStream_t)stream)) return AVT_OK;
  const int grid = ew_grid(nvec);
  if (256 % (C / 8) == 0 && bn_ew(kEwFwd))
    bn_apply_rw_dispatch<false>((const bf16_t*)x, scale, shift, (const bf16_t*)residual, rscale, rshift, (bf16_t*)out,
                                nullptr, rows, C, relu, (hipStream_t)stream);
  else if (256 % (C / 8) == 0)
    hipLaunchKernelGGL(bn_apply_kernel<true>, dim3(grid), dim3(256), 0, (hipStream_t)stream, (const bf16_t*)x, scale,
                       shift, (const bf16_t*)residual, rscale, rshift, (bf16_t*)out, nullptr, nvec, C, relu);
  else
    hipLaunchKernelGGL(bn_apply_kernel<false>, dim3(grid), dim3(256), 0, (hipStream_t)stream, (const bf16_t*)x, scale,
                       shift, (const bf16_t*)residual, rscale, rshift, (bf16_t*)out, nullptr, nvec, C, relu);
  return check_launch("bn_apply");
}

extern "C" int avt_bn_apply_mask(const void* x, const float* scale, const float* shift, const void* residual,
                                 const float* rscale, const float* rshift, void* out, void* mask, long long rows,
                                 int C, void* stream) {
  AVT_REQUIRE(x && scale && shift && out && mask, "bn_apply_mask: null pointer");
  AVT_REQUIRE(C % 8 == 0 && 256 % (C / 8) == 0, "bn_apply_mask: C=%d unsupported", C);
  AVT_REQUIRE((rscale == nullptr) == (rshift == nullptr), "bn_apply_mask: rscale/rshift must be both set or both null");
  const long long nvec = rows * C / 8;
  if (nvec == 0 || diag_skip(16, (hipStream_t)stream)) return AVT_OK;
  if (bn_ew(kEwFwd))
    bn_apply_rw_dispatch<true>((const bf16_t*)x, scale, shift, (const bf16_t*)residual, rscale, rshift, (bf16_t*)out,
                               (unsigned char*)mask, rows, C, 1, (hipStream_t)stream);
  else
    hipLaunchKernelGGL(bn_apply_kernel<true>, dim3(ew_grid(nvec)), dim3(256), 0, (hipStream_t)stream, (const bf16_t*)x,
                       scale, shift, (const bf16_t*)residual, rscale, rshift, (bf16_t*)out, (unsigned char*)mask, nvec,
                       C, 1);
  return check_launch("bn_apply_mask");
}

extern "C" int avt_bn_bwd_mask(const void* g, const void* mask, const avt_bn_bwd_target* t1,
                               const avt_bn_bwd_target* t2, long long rows, int C, void* stream) {
  AVT_REQUIRE(g && mask && t1, "bn_bwd_mask: null pointer");
  AVT_REQUIRE(C % 8 == 0 && C <= 2048 && 256 % (C / 8) == 0, "bn_bwd_mask: C=%d unsupported", C);
  AVT_REQUIRE(rows > 0, "bn_bwd_mask: empty input");
  const avt_bn_bwd_target* ts[2] = {t1, t2};
  for (int k = 0; k < (t2 ? 2 : 1); ++k) {
    const avt_bn_bwd_target* t = ts[k];
    AVT_REQUIRE(t->xc && t->mean && t->invstd && t->gamma && t->gc && t->workspace, "bn_bwd_mask: null target pointer");
    AVT_REQUIRE(((uintptr_t)t->workspace & 7) == 0, "bn_bwd_mask: workspace must be 8-byte aligned");
  }
  hipStream_t st = (hipStream_t)stream;
  double* acc = (double*)t1->workspace;
  float* k1 = bn_k1(acc);
  double* acc2 = t2 ? (double*)t2->workspace : nullptr;
  float* k1b = t2 ? bn_k1(acc2) : nullptr;
  MaskBwdArgs a{};
  a.g = (const bf16_t*)g;
  a.mk = (const unsigned char*)mask;
  a.xc = (const bf16_t*)t1->xc;
  a.mean = t1->mean;
  a.invstd = t1->invstd;
  a.acc = acc;
  if (t2) {
    a.xc2 = (const bf16_t*)t2->xc;
    a.mean2 = t2->mean;
    a.invstd2 = t2->invstd;
    a.acc2 = acc2;
  }
  a.rows = rows;
  a.C = C;
  const RowDeal d = reduce_deal(rows, C);
  a.rows_per_block = (int)d.rpb;
  const double inv_rows = 1.0 / (double)rows;
  MaskApplyArgs p{};
  p.g = a.g;
  p.mk = a.mk;
  p.xc = a.xc;
  p.mean = t1->mean;
  p.invstd = t1->invstd;
  p.gamma = t1->gamma;
  p.k1 = k1;
  p.k2 = k1 + C;
  p.gc = (bf16_t*)t1->gc;
  p.nvec = rows * C / 8;
  p.C = C;
  if (t2) {
    if (!diag_skip(8, st)) hipLaunchKernelGGL(bn_bwd_mask_reduce_kernel<true>, dim3(d.nblk), dim3(256), 0, st, a);
    bn_bwd_finalize_launch(st, C, inv_rows, true, acc, t1->dgamma, t1->dbeta, acc2, t2->dgamma, t2->dbeta);
    p.xc2 = (const bf16_t*)t2->xc;
    p.mean2 = t2->mean;
    p.invstd2 = t2->invstd;
    p.gamma2 = t2->gamma;
    p.k1b = k1b;
    p.k2b = k1b + C;
    p.gc2 = (bf16_t*)t2->gc;
    if (bn_ew(kEwMaskBwd))
      bn_bwd_mask_apply_rw_launch<true>(p, rows, st);
    else
      hipLaunchKernelGGL(bn_bwd_mask_apply_kernel<true>, dim3(ew_grid(p.nvec)), dim3(256), 0, st, p);
  } else {
    if (!diag_skip(8, st)) hipLaunchKernelGGL(bn_bwd_mask_reduce_kernel<false>, dim3(d.nblk), dim3(256), 0, st, a);
    bn_bwd_finalize_launch(st, C, inv_rows, true, acc, t1->dgamma, t1->dbeta);
    if (bn_ew(kEwMaskBwd))
      bn_bwd_mask_apply_rw_launch<false>(p, rows, st);
    else
      hipLaunchKernelGGL(bn_bwd_mask_apply_kernel<false>, dim3(ew_grid(p.nvec)), dim3(256), 0, st, p);
  }
  return check_launch("bn_bwd_mask");
}

// workspace: header + k1/k2 (2C floats) + the slots of up to `rows` rows (avt_common.h); any contents on entry
extern "C" size_t avt_bn_bwd_workspace(long long rows, int C) {
  if (rows < 0 || C <= 0) return 0;
  return ((size_t)kBnHdr + (size_t)C + (size_t)bn_slot_cap(rows) * C * 2) * sizeof(double);
}

extern "C" int avt_bn_bwd(const void* g, const void* y, const void* xc, const float* mean, const float* invstd,
                          const float* gamma, float* dgamma, float* dbeta, void* gc, void* gmask_out,
                          void* workspace, long long rows, int C, void* stream) {
  AVT_REQUIRE(g && xc && mean && invstd && gamma && gc && workspace, "bn_bwd: null pointer");
  AVT_REQUIRE(C % 8 == 0 && C <= 2048 && 256 % (C / 8) == 0, "bn_bwd: C=%d unsupported", C);
  AVT_REQUIRE(rows > 0, "bn_bwd: empty input");
  AVT_REQUIRE(((uintptr_t)workspace & 7) == 0, "bn_bwd: workspace must be 8-byte aligned");
  double* acc = (double*)workspace;
  float* k1 = bn_k1(acc);
  float* k2 = k1 + C;
  hipStream_t st = (hipStream_t)stream;
  if (!diag_skip(8, st))
    bn_bwd_reduce_launch((const bf16_t*)g, (const bf16_t*)y, nullptr, nullptr, (const bf16_t*)xc, mean, invstd, acc,
                         rows, C, st);
  bn_bwd_finalize_launch(st, C, 1.0 / (double)rows, true, acc, dgamma, dbeta);
  const long long nvec = rows * C / 8;
  if (bn_ew(kEwBwd))
    bn_bwd_apply_rw_launch((const bf16_t*)g, (const bf16_t*)y,
                           nullptr, nullptr, (const bf16_t*)xc, mean, invstd, gamma, k1, k2, (bf16_t*)gc,
                           (bf16_t*)gmask_out, rows, C, st);
  else
    hipLaunchKernelGGL(bn_bwd_apply_kernel<true>, dim3(ew_grid(nvec)), dim3(256), 0, st, (const bf16_t*)g, (const bf16_t*)y,
                       nullptr, nullptr, (const bf16_t*)xc, mean, invstd, gamma, k1, k2, (bf16_t*)gc,
                       (bf16_t*)gmask_out, nvec, C);
  return check_launch("bn_bwd");
}

// BN backward whose reductions were already accumulated into the workspace by a dgrad epilogue
// (avt_conv2d_dgrad_bn) over the pre-masked g': finalize (dgamma, dbeta, k1, k2 from the
// accumulator) + apply gc = gamma*invstd*(g' - k1 - xhat*k2).  Same workspace contract as avt_bn_bwd.
extern "C" int avt_bn_bwd_premasked(const void* gm, const void* xc, const float* mean, const float* invstd,
                                    const float* gamma, float* dgamma, float* dbeta, void* gc, void* workspace,
                                    long long rows, int C, void* stream) {
  AVT_REQUIRE(gm && xc && mean && invstd && gamma && gc && workspace, "bn_bwd_premasked: null pointer");
  AVT_REQUIRE(C % 8 == 0 && C <= 2048 && 256 % (C / 8) == 0, "bn_bwd_premasked: C=%d unsupported", C);
  AVT_REQUIRE(rows > 0, "bn_bwd_premasked: empty input");
  AVT_REQUIRE(((uintptr_t)workspace & 7) == 0, "bn_bwd_premasked: workspace must be 8-byte aligned");
  double* acc = (double*)workspace;
  float* k1 = bn_k1(acc);
  float* k2 = k1 + C;
  hipStream_t st = (hipStream_t)stream;
  bn_bwd_finalize_launch(st, C, 1.0 / (double)rows, true, acc, dgamma, dbeta);
  const long long nvec = rows * C / 8;
  if (bn_ew(kEwBwd))
    bn_bwd_apply_rw_launch((const bf16_t*)gm, nullptr,
                           nullptr, nullptr, (const bf16_t*)xc, mean, invstd, gamma, k1, k2, (bf16_t*)gc, nullptr, rows, C, st);
  else
    hipLaunchKernelGGL(bn_bwd_apply_kernel<true>, dim3(ew_grid(nvec)), dim3(256), 0, st, (const bf16_t*)gm, nullptr,
                       nullptr, nullptr, (const bf16_t*)xc, mean, invstd, gamma, k1, k2, (bf16_t*)gc, nullptr, nvec, C);
  return check_launch("bn_bwd_premasked");
}

// BN + ReLU backward with the mask recomputed from the pre-activation xc and the forward's
// (scale, shift): y is never read.  Same workspace contract as avt_bn_bwd.
extern "C" int avt_bn_relu_bwd(const void* g, const void* xc, const float* scale, const float* shift,
                               const float* mean, const float* invstd, const float* gamma, float* dgamma, float* dbeta,
                               void* gc, void* workspace, long long rows, int C, void* stream) {
  AVT_REQUIRE(g && xc && scale && shift && mean && invstd && gamma && gc && workspace, "bn_relu_bwd: null pointer");
  AVT_REQUIRE(C % 8 == 0 && C <= 2048 && 256 % (C / 8) == 0, "bn_relu_bwd: C=%d unsupported", C);
  AVT_REQUIRE(rows > 0, "bn_relu_bwd: empty input");
  AVT_REQUIRE(((uintptr_t)workspace & 7) == 0, "bn_relu_bwd: workspace must be 8-byte aligned");
  double* acc = (double*)workspace;
  float* k1 = bn_k1(acc);
  float* k2 = k1 + C;
  hipStream_t st = (hipStream_t)stream;
  if (!diag_skip(8, st))
    bn_bwd_reduce_launch((const bf16_t*)g, nullptr, scale, shift, (const bf16_t*)xc, mean, invstd, acc, rows, C, st);
  bn_bwd_finalize_launch(st, C, 1.0 / (double)rows, true, acc, dgamma, dbeta);
  const long long nvec = rows * C / 8;
  if (bn_ew(kEwBwd))
    bn_bwd_apply_rw_launch((const bf16_t*)g, nullptr, scale,
                           shift, (const bf16_t*)xc, mean, invstd, gamma, k1, k2, (bf16_t*)gc, nullptr, rows, C, st);
  else
    hipLaunchKernelGGL(bn_bwd_apply_kernel<true>, dim3(ew_grid(nvec)), dim3(256), 0, st, (const bf16_t*)g, nullptr, scale,
                       shift, (const bf16_t*)xc, mean, invstd, gamma, k1, k2, (bf16_t*)gc, nullptr, nvec, C);
  return check_launch("bn_relu_bwd");
}

static int ilog2(int v) {
  int l = 0;
  while ((1 << l) < v) ++l;
  return l;
}

extern "C" int avt_stem_bn_relu_maxpool_fwd(const void* c, const float* scale, const float* shift, void* y, void* idx,
                                            void* carg, int N, int H, int W, int C, void* stream) {
  AVT_REQUIRE(c && scale && shift && y && idx && carg, "stem_bn_relu_maxpool_fwd: null pointer");
  AVT_REQUIRE(C % 8 == 0 && 256 % (C / 8) == 0, "stem_bn_relu_maxpool_fwd: C=%d unsupported", C);
  AVT_REQUIRE(N > 0 && H > 0 && W > 0, "stem_bn_relu_maxpool_fwd: empty input");
  const int P = (H + 2 - 3) / 2 + 1, Q = (W + 2 - 3) / 2 + 1;
  hipLaunchKernelGGL(stem_bn_relu_maxpool_fwd_kernel, dim3(N * P), dim3(256), 0, (hipStream_t)stream,
                     (const bf16_t*)c, scale, shift, (bf16_t*)y, (unsigned char*)idx, (bf16_t*)carg, H, W, C,
                     ilog2(C / 8), P, Q);
  return check_launch("stem_bn_relu_maxpool_fwd");
}

extern "C" int avt_stem_maxpool_bn_relu_bwd(const void* gy, const void* idx, const void* carg, const void* c,
                                            const float* scale, const float* shift, const float* mean,
                                            const float* invstd, const float* gamma, float* dgamma, float* dbeta,
                                            void* gc, void* workspace, int N, int H, int W, int C, void* stream) {
  AVT_REQUIRE(gy && idx && carg && c && scale && shift && mean && invstd && gamma && gc && workspace,
              "stem_maxpool_bn_relu_bwd: null pointer");
  AVT_REQUIRE(C % 8 == 0 && C <= 2048 && 256 % (C / 8) == 0, "stem_maxpool_bn_relu_bwd: C=%d unsupported", C);
  AVT_REQUIRE((long long)((W + 1) / 2 + 1) * C * 6 <= kStemLdsBytes && (long long)2 * W * (C / 8) <= 6 * kStemBwdThreads,
              "stem_maxpool_bn_relu_bwd: W=%d C=%d too wide", W, C);
  AVT_REQUIRE(N > 0 && H > 0 && W > 0, "stem_maxpool_bn_relu_bwd: empty input");
  AVT_REQUIRE(((uintptr_t)workspace & 7) == 0, "stem_maxpool_bn_relu_bwd: workspace must be 8-byte aligned");
  const int P = (H + 2 - 3) / 2 + 1, Q = (W + 2 - 3) / 2 + 1;
  double* acc = (double*)workspace;
  float* k1 = bn_k1(acc);
  float* k2 = k1 + C;
  hipStream_t st = (hipStream_t)stream;
  bn_bwd_reduce_launch((const bf16_t*)gy, nullptr, scale, shift, (const bf16_t*)carg, mean, invstd, acc,
                       (long long)N * P * Q, C, st);
  bn_bwd_finalize_launch(st, C, 1.0 / ((double)N * H * W), true, acc, dgamma, dbeta);
  hipLaunchKernelGGL(stem_maxpool_bn_bwd_apply_kernel<false>, dim3(N * ((H + 1) / 2)), dim3(kStemBwdThreads),
                     (size_t)6 * Q * C, st, (const bf16_t*)gy,
                     (const unsigned char*)idx, (const bf16_t*)c, scale, shift, mean, invstd, gamma, k1, k2,
                     (bf16_t*)gc, H, W, C, ilog2(C / 8), P, Q);
  return check_launch("stem_maxpool_bn_relu_bwd");
}

// Eval-mode (running-statistics) stem backward: one pass gc = gamma*invstd * [fma(c, scale, shift) > 0] * (the gy of the
// windows whose argmax is the pixel).  dgamma / dbeta (optional) are summed over the pooled rows from (gy, carg) -- the
// train-mode entry's reduce -- through the fixed-order slots and added into the gradient by the finalize; both NULL:
// no workspace, nothing reduced.
extern "C" int avt_stem_maxpool_bn_relu_eval_bwd(const void* gy, const void* idx, const void* carg, const void* c,
                                                 const float* scale, const float* shift, const float* mean,
                                                 const float* invstd, const float* gamma, float* dgamma, float* dbeta,
                                                 void* gc, void* workspace, int N, int H, int W, int C, void* stream) {
  AVT_REQUIRE(gy && idx && c && scale && shift && invstd && gamma && gc, "stem_maxpool_bn_relu_eval_bwd: null pointer");
  AVT_REQUIRE(C % 8 == 0 && C <= 2048 && 256 % (C / 8) == 0, "stem_maxpool_bn_relu_eval_bwd: C=%d unsupported", C);
  AVT_REQUIRE((long long)((W + 1) / 2 + 1) * C * 6 <= kStemLdsBytes && (long long)2 * W * (C / 8) <= 6 * kStemBwdThreads,
              "stem_maxpool_bn_relu_eval_bwd: W=%d C=%d too wide", W, C);
  AVT_REQUIRE(N > 0 && H > 0 && W > 0, "stem_maxpool_bn_relu_eval_bwd: empty input");
  const bool wants = dgamma || dbeta;
  AVT_REQUIRE(!wants || (carg && mean && workspace && ((uintptr_t)workspace & 7) == 0),
              "stem_maxpool_bn_relu_eval_bwd: dgamma/dbeta need carg, mean and an 8-byte aligned workspace");
  const int P = (H + 2 - 3) / 2 + 1, Q = (W + 2 - 3) / 2 + 1;
  hipStream_t st = (hipStream_t)stream;
  if (wants) {
    double* acc = (double*)workspace;
    bn_bwd_reduce_launch((const bf16_t*)gy, nullptr, scale, shift, (const bf16_t*)carg, mean, invstd, acc,
                         (long long)N * P * Q, C, st);
    // (k1 / k2, the train-mode rule's means: written, not used here)
    bn_bwd_finalize_launch(st, C, 1.0 / ((double)N * H * W), false, acc, dgamma, dbeta);
  }
  hipLaunchKernelGGL(stem_maxpool_bn_bwd_apply_kernel<true>, dim3(N * ((H + 1) / 2)), dim3(kStemBwdThreads),
                     (size_t)6 * Q * C, st, (const bf16_t*)gy, (const unsigned char*)idx, (const bf16_t*)c, scale, shift,
                     nullptr, invstd, gamma, nullptr, nullptr, (bf16_t*)gc, H, W, C, ilog2(C / 8), P, Q);
  return check_launch("stem_maxpool_bn_relu_eval_bwd");
}
