// Frame transform of the reference's dataset on the device (datasets/dataloader.py:47-62; SURVEY
// §8f rank 4): Resize(short side, PIL BICUBIC) -> crop (Random/Center) -> optional horizontal flip
// -> ToTensor -> Normalize(mean, std), from decoded RGB uint8 frames to the float32 [n][3][S][S]
// tensor the reference's DataLoader yields.
//
// The resize is Pillow's separable fixed-point resampler (Image.resize(size, BICUBIC), Pillow
// 12.2.0 in this image): per output index, weights of the a = -0.5 bicubic kernel stretched by the
// downscale factor, normalised in double, rounded to int32 with 22 fraction bits; a horizontal pass
// into an 8-bit intermediate, then a vertical pass, each accumulated in int32 from 1 << 21, shifted
// and clipped to [0, 255].  The coefficients are computed on the device in double precision with
// contraction off (Pillow's x86-64 build does a separate multiply and add), so the output is
// bit-identical to Pillow.  Only the crop window's columns (horizontal pass) and rows (vertical
// pass) are computed: every output pixel of the resampler is independent of the others.
//
// Two launches per batch: (1) horizontal pass, one thread per crop column, rows restricted to those
// the crop's vertical taps read, written as planar uint8 [n][3][Hmax][S]; (2) vertical pass + crop +
// flip + /255 + normalise, one thread per output pixel column, coalesced fp32 stores.  HBM-bound:
// the source bytes once (L2 catches the tap overlap), 3 B per intermediate pixel, 12 B per output.
#include "avt_common.h"

namespace avt {

constexpr int FR_PREC = 22;  // Pillow: PRECISION_BITS = 32 - 8 - 2
constexpr int FR_KMAX = 32;  // taps per output index: downscale factor <= 7.5
constexpr int FR_T = 256;    // threads per block = max crop size

struct FrameDesc {  // the int64[8] row of the descriptor table, as passed in
  long long off, H, W, rh, rw, ci, cj, flip;
};

__device__ __forceinline__ double bicubic_w(double x) {
#pragma clang fp contract(off)
  const double a = -0.5;
  if (x < 0.0) x = -x;
  if (x < 1.0) return ((a + 2.0) * x - (a + 3.0)) * x * x + 1;
  if (x < 2.0) return (((x - 5) * x + 8) * x - 4) * a;
  return 0.0;
}

// Pillow precompute_coeffs (box = whole image) + normalize_coeffs_8bpc for output index xx.
// Returns the tap count; k[0..count) are the fixed-point weights, *first the first source index.
__device__ int frame_coeffs(int in_size, int out_size, int xx, int* k, int* first) {
#pragma clang fp contract(off)
  const double scale = (double)in_size / (double)out_size;
  const double filterscale = scale < 1.0 ? 1.0 : scale;
  const double support = 2.0 * filterscale;
  const double center = ((double)xx + 0.5) * scale;
  const double ss = 1.0 / filterscale;
  int xmin = (int)(center - support + 0.5);
  if (xmin < 0) xmin = 0;
  int xmax = (int)(center + support + 0.5);
  if (xmax > in_size) xmax = in_size;
  xmax -= xmin;
  if (xmax > FR_KMAX) xmax = FR_KMAX;  // only past the host-checked factor 7.5: wrong, never out of bounds
  double w[FR_KMAX];
  double ww = 0.0;
  for (int x = 0; x < xmax; ++x) {
    w[x] = bicubic_w(((double)(x + xmin) - center + 0.5) * ss);
    ww += w[x];
  }
  for (int x = 0; x < xmax; ++x) {
    const double v = ww != 0.0 ? w[x] / ww : w[x];
    const double f = v * (double)(1 << FR_PREC);
    k[x] = v < 0 ? (int)(-0.5 + f) : (int)(0.5 + f);
  }
  *first = xmin;
  return xmax;
}

__device__ __forceinline__ int clip8(int ss) {
  const int v = ss >> FR_PREC;
  return v < 0 ? 0 : (v > 255 ? 255 : v);
}

// (1) horizontal pass: tmp[img][c][y][x] for crop columns x (resized column cj + x) and the rows y
// the vertical taps of crop rows ci .. ci+S-1 read.
__global__ __launch_bounds__(FR_T) void frames_hpass_kernel(const unsigned char* __restrict__ src,
                                                            const long long* __restrict__ desc, int S, int Hmax,
                                                            int rows_per_block, unsigned char* __restrict__ tmp) {
  __shared__ int kk[FR_KMAX][FR_T];
  __shared__ int yr[2];
  const int img = blockIdx.y, x = threadIdx.x;
  const FrameDesc d = reinterpret_cast<const FrameDesc*>(desc)[img];
  const int H = (int)d.H, W = (int)d.W;
  if (threadIdx.x < 2) {  // source rows read by the vertical taps of the first / last crop row
    int kt[FR_KMAX], f;
    const int yy = (int)d.ci + (threadIdx.x ? S - 1 : 0);
    const int n = frame_coeffs(H, (int)d.rh, yy, kt, &f);
    yr[threadIdx.x] = threadIdx.x ? f + n : f;
  }
  int xmin = 0, cnt = 0;
  if (x < S) {
    int kt[FR_KMAX];
    cnt = frame_coeffs(W, (int)d.rw, (int)d.cj + x, kt, &xmin);
    for (int t = 0; t < cnt; ++t) kk[t][x] = kt[t];
  }
  __syncthreads();
  const int y0 = max(yr[0], blockIdx.x * rows_per_block), y1 = min(yr[1], (blockIdx.x + 1) * rows_per_block);
  if (x >= S) return;
  const unsigned char* im = src + d.off;
  const size_t plane = (size_t)Hmax * S;
  unsigned char* o = tmp + (size_t)img * 3 * plane;
  for (int y = y0; y < y1; ++y) {
    const unsigned char* row = im + ((size_t)y * W + xmin) * 3;
    int s0 = 1 << (FR_PREC - 1), s1 = s0, s2 = s0;
    for (int t = 0; t < cnt; ++t) {
      const int w = kk[t][x];
      s0 += (int)row[3 * t + 0] * w;
      s1 += (int)row[3 * t + 1] * w;
      s2 += (int)row[3 * t + 2] * w;
    }
    const size_t at = (size_t)y * S + x;
    o[at] = (unsigned char)clip8(s0);
    o[plane + at] = (unsigned char)clip8(s1);
    o[2 * plane + at] = (unsigned char)clip8(s2);
  }
}

// (2) vertical pass of crop row i + horizontal flip + ToTensor + Normalize -> out[img][c][i][j].
// tpc = frames per clip: frame img = clip * tpc + k goes to out[clip][c][k][i][j] (NCTHW; tpc = 1 is
// the plain [n][3][S][S]).  u8, when given, also takes the 8-bit pixels, planar [img][c][i][j].
__global__ __launch_bounds__(FR_T) void frames_vpass_kernel(const unsigned char* __restrict__ tmp,
                                                            const long long* __restrict__ desc, int S, int Hmax,
                                                            float m0, float m1, float m2, float s0, float s1,
                                                            float s2, int tpc, float* __restrict__ out,
                                                            unsigned char* __restrict__ u8) {
  __shared__ int kk[FR_KMAX];
  __shared__ int hdr[2];
  const int i = blockIdx.x, img = blockIdx.y, j = threadIdx.x;
  const FrameDesc d = reinterpret_cast<const FrameDesc*>(desc)[img];
  if (threadIdx.x == 0) {
    int kt[FR_KMAX], f;
    const int n = frame_coeffs((int)d.H, (int)d.rh, (int)d.ci + i, kt, &f);
    for (int t = 0; t < n; ++t) kk[t] = kt[t];
    hdr[0] = f;
    hdr[1] = n;
  }
  __syncthreads();
  if (j >= S) return;
  const int ymin = hdr[0], cnt = hdr[1];
  const int x = d.flip ? S - 1 - j : j;
  const size_t plane = (size_t)Hmax * S;
  const unsigned char* t0 = tmp + (size_t)img * 3 * plane + (size_t)ymin * S + x;
  int a0 = 1 << (FR_PREC - 1), a1 = a0, a2 = a0;
  for (int t = 0; t < cnt; ++t) {
    const int w = kk[t];
    a0 += (int)t0[(size_t)t * S] * w;
    a1 += (int)t0[plane + (size_t)t * S] * w;
    a2 += (int)t0[2 * plane + (size_t)t * S] * w;
  }
  // ToTensor (x / 255) then Normalize ((x - mean) / std), float32 as torchvision does it
  const size_t px = (size_t)S * S, at = (size_t)i * S + j;
  const int clip = img / tpc, k = img - clip * tpc;
  float* o = out + ((size_t)clip * 3 * tpc + k) * px + at;
  const size_t cs = (size_t)tpc * px;
  const int v0 = clip8(a0), v1 = clip8(a1), v2 = clip8(a2);
  o[0] = ((float)v0 / 255.f - m0) / s0;
  o[cs] = ((float)v1 / 255.f - m1) / s1;
  o[2 * cs] = ((float)v2 / 255.f - m2) / s2;
  if (u8) {
    unsigned char* b = u8 + (size_t)img * 3 * px + at;
    b[0] = (unsigned char)v0;
    b[px] = (unsigned char)v1;
    b[2 * px] = (unsigned char)v2;
  }
}

// ---- colour jitter of the two-view clip transform (datasets/dataloader.py:165-170) ----
// torchvision's ColorJitter on its PIL path, i.e. Pillow's 8-bit arithmetic, restated and pinned against
// Pillow in tests/test_clip_cpu.py (both hue conversions over all 2^24 inputs).  Contraction stays off:
// Pillow's build rounds every multiply and add on its own.
constexpr int CJ_T = 512;     // threads of the jitter block (one block per frame)
constexpr int CJ_MAXOPS = 4;  // brightness, contrast, saturation, hue: each at most once

__device__ __forceinline__ int gray_l(int r, int g, int b) {  // convert("L")
  return (19595 * r + 38470 * g + 7471 * b + 0x8000) >> 16;
}

// Image.blend(deg, img, f) on one 8-bit channel: fp32, truncated; clipped when f is outside [0, 1]
__device__ __forceinline__ int blend8(int deg, int img, float f, bool clip) {
#pragma clang fp contract(off)
  const float d = (float)deg;
  const float df = (float)img - d;
  const float fd = f * df;
  const float tmp = d + fd;
  if (clip) {
    if (tmp <= 0.f) return 0;
    if (tmp >= 255.f) return 255;
  }
  return (int)tmp;
}

__device__ __forceinline__ int clipi8(int v) { return v < 0 ? 0 : (v > 255 ? 255 : v); }

// convert("HSV") of one pixel: float h, s; the hue's constants are doubles
__device__ void rgb_to_hsv(int r, int g, int b, int* uh, int* us, int* uv) {
#pragma clang fp contract(off)
  const int maxc = max(r, max(g, b)), minc = min(r, min(g, b));
  *uv = maxc;
  if (minc == maxc) {
    *uh = 0;
    *us = 0;
    return;
  }
  const float cr = (float)(maxc - minc);
  const float s = cr / (float)maxc;
  const float rc = (float)(maxc - r) / cr, gc = (float)(maxc - g) / cr, bc = (float)(maxc - b) / cr;
  float h;
  if (r == maxc) {
    h = bc - gc;
  } else if (g == maxc) {
    const double t = 2.0 + (double)rc;
    h = (float)(t - (double)bc);
  } else {
    const double t = 4.0 + (double)gc;
    h = (float)(t - (double)rc);
  }
  const double q = (double)h / 6.0;
  const double w = q + 1.0;       // in (0.83, 1.84)
  h = (float)(w - floor(w));      // fmod(w, 1.0), exact
  *uh = clipi8((int)((double)h * 255.0));
  *us = clipi8((int)((double)s * 255.0));
}

// convert("RGB") of one HSV pixel: sector and remainder of h * 6 / 255, p / q / t rounded half away from 0
__device__ void hsv_to_rgb(int h, int s, int v, int* r, int* g, int* b) {
#pragma clang fp contract(off)
  if (s == 0) {
    *r = *g = *b = v;
    return;
  }
  const double h6 = (double)h * 6.0 / 255.0;
  const int i = (int)floor(h6);
  const double f = (double)(float)(h6 - (double)i);
  const double fs = (double)(float)((double)s / 255.0);
  const double dv = (double)v;
  const double fsf = fs * f;
  const double omf = 1.0 - f;
  const double fso = fs * omf;
  const double ap = 1.0 - fs, aq = 1.0 - fsf, at = 1.0 - fso;
  const double xp = dv * ap, xq = dv * aq, xt = dv * at;  // all >= 0
  const int p = clipi8((int)floor(xp + 0.5)), q = clipi8((int)floor(xq + 0.5)), t = clipi8((int)floor(xt + 0.5));
  switch (i % 6) {
    case 0: *r = v, *g = t, *b = p; break;
    case 1: *r = q, *g = v, *b = p; break;
    case 2: *r = p, *g = v, *b = t; break;
    case 3: *r = p, *g = q, *b = v; break;
    case 4: *r = t, *g = p, *b = v; break;
    default: *r = v, *g = p, *b = q; break;
  }
}

struct JitterOps {
  int n;
  int kind[CJ_MAXOPS];
  float f[CJ_MAXOPS];  // Pillow's blend takes its factor as a C float
  int shift;           // the HUE op's 8-bit offset
};

// ops [from, to) on one pixel; `mean` is the frame's contrast mean (used by a CONTRAST op in the range)
__device__ __forceinline__ void jitter_apply(const JitterOps& J, int from, int to, int mean, int* r, int* g, int* b) {
  for (int o = from; o < to; ++o) {
    const float f = J.f[o];
    const bool clip = !(f >= 0.f && f <= 1.f);
    switch (J.kind[o]) {
      case AVT_JITTER_BRIGHTNESS:
        *r = blend8(0, *r, f, clip), *g = blend8(0, *g, f, clip), *b = blend8(0, *b, f, clip);
        break;
      case AVT_JITTER_CONTRAST:
        *r = blend8(mean, *r, f, clip), *g = blend8(mean, *g, f, clip), *b = blend8(mean, *b, f, clip);
        break;
      case AVT_JITTER_SATURATION: {
        const int l = gray_l(*r, *g, *b);
        *r = blend8(l, *r, f, clip), *g = blend8(l, *g, f, clip), *b = blend8(l, *b, f, clip);
        break;
      }
      case AVT_JITTER_HUE: {
        int h, s, v;
        rgb_to_hsv(*r, *g, *b, &h, &s, &v);
        h = (h + J.shift) & 255;
        hsv_to_rgb(h, s, v, r, g, b);
        break;
      }
      default:
        break;  // unknown kinds are refused by the caller
    }
  }
}

// One block per frame: the S2 x S2 crop of the frame's planar 8-bit view 1, through the clip's op chain,
// into jit[img] as packed RGB (the horizontal pass's source layout), plus the descriptor row of the
// view-2 resize (S2 -> S, no crop).  A CONTRAST op needs sum(L) of the whole frame after the ops before
// it: pass A runs those ops, stores the pixels and sums L in integers (block reduction, plain stores,
// no atomics: an integer sum does not depend on its order); pass B re-reads each thread's own pixels
// and runs the rest.
__global__ __launch_bounds__(CJ_T) void clip_jitter_kernel(const unsigned char* __restrict__ u8,
                                                           const avt_clip_view2* __restrict__ view2, int S, int S2,
                                                           int tpc, unsigned char* jit, long long* desc2) {
  __shared__ unsigned red[CJ_T / 64];
  const int img = blockIdx.x;
  const avt_clip_view2 V = view2[img / tpc];
  JitterOps J;
  J.n = min(max(V.nops, 0), CJ_MAXOPS);
  J.shift = 0;
  int cpos = J.n;
  for (int o = 0; o < CJ_MAXOPS; ++o) {
    J.kind[o] = o < J.n ? V.ops[o].kind : -1;
    J.f[o] = o < J.n ? (float)V.ops[o].factor : 1.f;
    if (J.kind[o] == AVT_JITTER_CONTRAST && cpos == J.n) cpos = o;
    if (J.kind[o] == AVT_JITTER_HUE) {  // int(h * 255) in double, toward zero; |h| <= 0.5 (clamped: a bad table)
      const double h = fmin(fmax(V.ops[o].factor, -0.5), 0.5);
      J.shift = (int)(h * 255.0) + 256;
    }
  }
  // the caller keeps the crop inside the view; clamped so that a bad table cannot read outside it
  const int top = min(max(V.crop_top, 0), S - S2), left = min(max(V.crop_left, 0), S - S2);
  const size_t px = (size_t)S * S;
  const int n2 = S2 * S2;
  const unsigned char* in = u8 + (size_t)img * 3 * px + (size_t)top * S + left;
  unsigned char* o = jit + (size_t)img * 3 * n2;
  if (threadIdx.x == 0) {
    long long* d = desc2 + (size_t)img * 8;
    d[0] = (long long)img * 3 * n2;
    d[1] = S2, d[2] = S2, d[3] = S, d[4] = S, d[5] = 0, d[6] = 0;
    d[7] = V.flip ? 1 : 0;
  }
  unsigned sum = 0;  // <= 255 * 179^2
  for (int p = threadIdx.x; p < n2; p += CJ_T) {
    const int y = p / S2, x = p - y * S2;
    const unsigned char* q = in + (size_t)y * S + x;
    int r = q[0], g = q[px], b = q[2 * px];
    jitter_apply(J, 0, cpos, 0, &r, &g, &b);
    if (cpos < J.n) sum += (unsigned)gray_l(r, g, b);
    o[3 * p + 0] = (unsigned char)r, o[3 * p + 1] = (unsigned char)g, o[3 * p + 2] = (unsigned char)b;
  }
  if (cpos == J.n) return;  // uniform over the block
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) sum += __shfl_xor(sum, d, 64);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = sum;
  __syncthreads();
  unsigned total = 0;
  for (int w = 0; w < CJ_T / 64; ++w) total += red[w];
  int mean;
  {
#pragma clang fp contract(off)
    const double m = (double)total / (double)n2;
    mean = (int)(m + 0.5);
  }
  for (int p = threadIdx.x; p < n2; p += CJ_T) {  // this thread's own stores of pass A
    int r = o[3 * p + 0], g = o[3 * p + 1], b = o[3 * p + 2];
    jitter_apply(J, cpos, J.n, mean, &r, &g, &b);
    o[3 * p + 0] = (unsigned char)r, o[3 * p + 1] = (unsigned char)g, o[3 * p + 2] = (unsigned char)b;
  }
}

}  // namespace avt

using namespace avt;

// The two passes of the resampler over n frames: (1) horizontal, (2) vertical + crop + flip + normalise into
// out (frame i = clip * tpc + k at [clip][c][k][.][.]) and, when u8 is given, the 8-bit pixels as well.
static int resize_launch(const void* src, const long long* desc, int n, int S, int Hmax, void* tmp, const float* mean,
                         const float* std, int tpc, float* out, void* u8, hipStream_t stream) {
  const int rows_per_block = 32;
  hipLaunchKernelGGL(frames_hpass_kernel, dim3((Hmax + rows_per_block - 1) / rows_per_block, n), dim3(FR_T), 0,
                     stream, (const unsigned char*)src, desc, S, Hmax, rows_per_block, (unsigned char*)tmp);
  int rc = check_launch("frames_hpass");
  if (rc != AVT_OK) return rc;
  hipLaunchKernelGGL(frames_vpass_kernel, dim3(S, n), dim3(FR_T), 0, stream, (const unsigned char*)tmp, desc, S, Hmax,
                     mean[0], mean[1], mean[2], std[0], std[1], std[2], tpc, out, (unsigned char*)u8);
  return check_launch("frames_vpass");
}

// src: decoded RGB frames, uint8 HWC, packed at byte offsets desc[i].off; desc: DEVICE int64
// [n][8] = {off, H, W, resized_h, resized_w, crop_top, crop_left, flip}; tmp: device scratch of
// n * 3 * Hmax * S bytes (Hmax >= every H); mean / std: HOST float[3]; out: float32 [n][3][S][S].
// The host-side checks (sizes, downscale factor <= 7.5 so that <= 32 taps, crop inside the resized
// image, Hmax >= H) are the caller's (avt_amd.frames); given them the kernels read only inside each
// frame and write only inside tmp / out.
extern "C" int avt_frames_transform(const void* src, const long long* desc, int n, int S, int Hmax, void* tmp,
                                    const float* mean, const float* std, float* out, void* stream) {
  AVT_REQUIRE(src && desc && tmp && mean && std && out, "frames_transform: null pointer");
  AVT_REQUIRE(n >= 1 && S >= 1 && S <= FR_T && Hmax >= 1, "frames_transform: need n >= 1, 1 <= S <= 256");
  return resize_launch(src, desc, n, S, Hmax, tmp, mean, std, 1, out, nullptr, (hipStream_t)stream);
}

// ---- two-view clip transform (datasets/dataloader.py:155-181, 260-263) ----
// Workspace layout (two_views): [desc2: n x 8 int64][tmp: n*3*Hmax*S][u8: n*3*S*S][jit: n*S2*S2*3]
// [tmp2: n*3*S2*S], each part rounded up to 16 bytes; one view needs tmp alone.
static size_t up16(size_t v) { return (v + 15) & ~(size_t)15; }

extern "C" int avt_clip_crop2(int S) { return (int)(S * 0.7); }

extern "C" size_t avt_clip_workspace_bytes(int b, int t, int S, int Hmax, int two_views) {
  if (b < 1 || t < 1 || S < 1 || S > FR_T || Hmax < 1) return 0;
  const size_t n = (size_t)b * t, S2 = (size_t)avt_clip_crop2(S);
  size_t bytes = up16(n * 3 * Hmax * S);
  if (two_views) bytes += up16(n * 64) + up16(n * 3 * S * S) + up16(n * S2 * S2 * 3) + up16(n * 3 * S2 * S);
  return bytes;
}

extern "C" int avt_clip_transform(const void* src, const long long* desc, const avt_clip_view2* view2, int b, int t,
                                  int S, int Hmax, void* workspace, size_t ws_bytes, const float* mean,
                                  const float* std, float* frames, float* augmented, void* stream) {
  AVT_REQUIRE(src && desc && workspace && mean && std && frames, "clip_transform: null pointer");
  AVT_REQUIRE((view2 != nullptr) == (augmented != nullptr),
              "clip_transform: view2 and augmented go together (both, or neither for one view)");
  AVT_REQUIRE(b >= 1 && t >= 1 && S >= 1 && S <= FR_T && Hmax >= 1 && (long long)b * t <= 65535,
              "clip_transform: need b, t >= 1, b * t <= 65535, 1 <= S <= 256, Hmax >= 1");
  const int two = view2 != nullptr, S2 = avt_clip_crop2(S);
  AVT_REQUIRE(!two || S2 >= 1, "clip_transform: the second view's crop int(0.7 S) is empty");
  AVT_REQUIRE(ws_bytes >= avt_clip_workspace_bytes(b, t, S, Hmax, two),
              "clip_transform: workspace of %zu bytes, need avt_clip_workspace_bytes() = %zu", ws_bytes,
              avt_clip_workspace_bytes(b, t, S, Hmax, two));
  AVT_REQUIRE((uintptr_t)workspace % 16 == 0 && (uintptr_t)desc % 8 == 0 && (uintptr_t)view2 % 8 == 0 &&
                  (uintptr_t)frames % 4 == 0 && (uintptr_t)augmented % 4 == 0,
              "clip_transform: misaligned pointer (workspace 16, desc / view2 8, frames / augmented 4 bytes)");
  const hipStream_t st = (hipStream_t)stream;
  const int n = b * t;
  unsigned char* w = (unsigned char*)workspace;
  long long* desc2 = (long long*)w;
  if (two) w += up16((size_t)n * 64);
  unsigned char* tmp = w;
  w += up16((size_t)n * 3 * Hmax * S);
  unsigned char* u8 = two ? w : nullptr;
  int rc = resize_launch(src, desc, n, S, Hmax, tmp, mean, std, t, frames, u8, st);
  if (rc != AVT_OK || !two) return rc;
  w += up16((size_t)n * 3 * S * S);
  unsigned char* jit = w;
  w += up16((size_t)n * S2 * S2 * 3);
  unsigned char* tmp2 = w;
  hipLaunchKernelGGL(clip_jitter_kernel, dim3(n), dim3(CJ_T), 0, st, (const unsigned char*)u8, view2, S, S2, t, jit,
                     desc2);
  rc = check_launch("clip_jitter");
  if (rc != AVT_OK) return rc;
  return resize_launch(jit, desc2, n, S, S2, tmp2, mean, std, t, augmented, nullptr, st);
}
