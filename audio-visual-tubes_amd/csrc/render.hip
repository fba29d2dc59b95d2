// The qualitative output of the reference's entry scripts, batched on the device: one block per frame.
//
// Restates save_image (visualize.py:46-50, train_3D.py:73-81, flow.py:71-79) and save_labels (flow.py:80-84):
//   image = normalize_img(image)                                   (one frame: its global min/max, fp32)
//   temp  = cv2.applyColorMap(np.uint8(gt_map * 128), COLORMAP_JET);  temp2 = ...(np.uint8(pred * 255), ...)
//   np.uint8(np.add((image[0] * 255).transpose(1, 2, 0) * 0.4, np.add(temp * 0.5, temp2 * 0.5) * 0.6))
// with applyColorMap(x) := lut[x], a [256][3] u8 table the caller passes.
//
// Arithmetic (numpy 2.x evaluating that expression gives the same bytes): the frame term stays fp32 -- a correctly
// rounded divide, then two separately rounded products -- the colour term is fp64 (u8 * python float), the sum is
// fp64 and np.uint8 truncates it.  No product is contracted into an FMA, in either precision.  Out-of-range sums
// saturate to [0, 255] (numpy's cast of them is undefined); a map value outside [0, 255] after scaling is clamped.
// Channel ch of the table is added to channel ch of the frame, as the reference adds cv2's BGR table to an RGB frame.
#include "avt_common.h"
#include "exact_fp.h"

namespace avt {

constexpr int RD_T = 1024;

struct OverlayArgs {
  const float* img;   // [N][3][H][W]
  const float* map0;  // [N][H][W] or NULL
  const float* map1;  // [N][H][W] or NULL (only with map0)
  const unsigned char* lut;  // [256][3]
  unsigned char* out;        // [N][H][W][3]
  int HW;
  float scale0, scale1, wimg;
  double w0;
  int vec_in;  // H*W % 4 == 0 and img, map0, map1 16-byte aligned: float4 loads
};

__device__ __forceinline__ int lut_index(float v, float scale) {
  const float p = mul_rn(v, scale);
  return (int)fminf(fmaxf(p, 0.f), 255.f);  // truncation; NaN -> 0
}

// the three output bytes of one pixel: x[ch] the frame's channels, m0 / m1 the layers' map values
template <int LAYERS>
__device__ __forceinline__ void blend_pixel(const OverlayArgs& a, const unsigned char* lut, float vmin, float rng,
                                            const float x[3], float m0, float m1, unsigned char o[3]) {
  int i0 = 0, i1 = 0;
  if (LAYERS >= 1) i0 = 3 * lut_index(m0, a.scale0);
  if (LAYERS == 2) i1 = 3 * lut_index(m1, a.scale1);
#pragma unroll
  for (int ch = 0; ch < 3; ++ch) {
    const float n = rng != 0.f ? div_rn(sub_rn(x[ch], vmin), rng) : x[ch];
    const float f = mul_rn(mul_rn(n, 255.f), a.wimg);
    if (LAYERS == 0) {
      o[ch] = (unsigned char)(int)fminf(fmaxf(f, 0.f), 255.f);
    } else {
      double c;
      if (LAYERS == 2)
        c = add_rn(mul_rn((double)lut[i0 + ch], 0.5), mul_rn((double)lut[i1 + ch], 0.5));
      else
        c = (double)lut[i0 + ch];
      const double s = add_rn((double)f, mul_rn(c, a.w0));
      o[ch] = (unsigned char)(int)fmin(fmax(s, 0.0), 255.0);  // saturate, then truncate
    }
  }
}

template <int LAYERS>
__global__ __launch_bounds__(RD_T) void render_overlay_kernel(OverlayArgs a) {
  __shared__ unsigned char lut[768];
  __shared__ float fred[2][RD_T / 64];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int HW = a.HW;
  const size_t frame = blockIdx.x;
  const float* x = a.img + frame * 3 * (size_t)HW;
  if (LAYERS > 0)
    for (int i = tid; i < 768; i += RD_T) lut[i] = a.lut[i];
  // phase 1: the frame's min / max over its 3 H W values
  float mn = INFINITY, mx = -INFINITY;
  if (a.vec_in) {
    const f32x4* x4 = reinterpret_cast<const f32x4*>(x);
    for (int i = tid; i < 3 * (HW / 4); i += RD_T) {
      const f32x4 v = x4[i];
      mn = fminf(fminf(mn, v.x), fminf(v.y, fminf(v.z, v.w)));
      mx = fmaxf(fmaxf(mx, v.x), fmaxf(v.y, fmaxf(v.z, v.w)));
    }
  } else {
    for (int i = tid; i < 3 * HW; i += RD_T) {
      const float v = x[i];
      mn = fminf(mn, v);
      mx = fmaxf(mx, v);
    }
  }
  for (int o = 32; o >= 1; o >>= 1) {
    mn = fminf(mn, __shfl_xor(mn, o, 64));
    mx = fmaxf(mx, __shfl_xor(mx, o, 64));
  }
  if (lane == 0) {
    fred[0][wv] = mn;
    fred[1][wv] = mx;
  }
  __syncthreads();
  float vmin = fred[0][0], vmax = fred[1][0];
  for (int k = 1; k < RD_T / 64; ++k) {
    vmin = fminf(vmin, fred[0][k]);
    vmax = fmaxf(vmax, fred[1][k]);
  }
  const float rng = sub_rn(vmax, vmin);
  // phase 2: the blend; a thread owns 4 consecutive pixels = 12 output bytes
  const float* m0 = LAYERS >= 1 ? a.map0 + frame * (size_t)HW : nullptr;
  const float* m1 = LAYERS == 2 ? a.map1 + frame * (size_t)HW : nullptr;
  unsigned char* out = a.out + frame * 3 * (size_t)HW;
  for (int g = tid; g < HW / 4; g += RD_T) {
    const int p = 4 * g;
    float xs[3][4], v0[4] = {0.f, 0.f, 0.f, 0.f}, v1[4] = {0.f, 0.f, 0.f, 0.f};
    if (a.vec_in) {
#pragma unroll
      for (int ch = 0; ch < 3; ++ch) {
        const f32x4 v = *reinterpret_cast<const f32x4*>(x + (size_t)ch * HW + p);
        xs[ch][0] = v.x, xs[ch][1] = v.y, xs[ch][2] = v.z, xs[ch][3] = v.w;
      }
      if (LAYERS >= 1) {
        const f32x4 v = *reinterpret_cast<const f32x4*>(m0 + p);
        v0[0] = v.x, v0[1] = v.y, v0[2] = v.z, v0[3] = v.w;
      }
      if (LAYERS == 2) {
        const f32x4 v = *reinterpret_cast<const f32x4*>(m1 + p);
        v1[0] = v.x, v1[1] = v.y, v1[2] = v.z, v1[3] = v.w;
      }
    } else {
#pragma unroll
      for (int k = 0; k < 4; ++k) {
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) xs[ch][k] = x[(size_t)ch * HW + p + k];
        if (LAYERS >= 1) v0[k] = m0[p + k];
        if (LAYERS == 2) v1[k] = m1[p + k];
      }
    }
    unsigned char b[12];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const float px[3] = {xs[0][k], xs[1][k], xs[2][k]};
      blend_pixel<LAYERS>(a, lut, vmin, rng, px, v0[k], v1[k], b + 3 * k);
    }
    unsigned char* dst = out + 3 * (size_t)p;
    if ((reinterpret_cast<uintptr_t>(dst) & 3u) == 0) {
      unsigned* d4 = reinterpret_cast<unsigned*>(dst);
#pragma unroll
      for (int k = 0; k < 3; ++k)
        d4[k] = (unsigned)b[4 * k] | ((unsigned)b[4 * k + 1] << 8) | ((unsigned)b[4 * k + 2] << 16) |
                ((unsigned)b[4 * k + 3] << 24);
    } else {
#pragma unroll
      for (int k = 0; k < 12; ++k) dst[k] = b[k];
    }
  }
  // the H W % 4 pixels left over
  for (int p = (HW & ~3) + tid; p < HW; p += RD_T) {
    const float px[3] = {x[p], x[(size_t)HW + p], x[2 * (size_t)HW + p]};
    unsigned char b[3];
    blend_pixel<LAYERS>(a, lut, vmin, rng, px, LAYERS >= 1 ? m0[p] : 0.f, LAYERS == 2 ? m1[p] : 0.f, b);
    out[3 * (size_t)p] = b[0];
    out[3 * (size_t)p + 1] = b[1];
    out[3 * (size_t)p + 2] = b[2];
  }
}

}  // namespace avt

using namespace avt;

// img [N][3][H][W] fp32 frames -> out [N][H][W][3] u8: each frame min-max normalised over its own 3 H W values,
// times 255 and wimg (fp32), plus the colour-mapped layers (fp64): (lut[u8(map0 scale0)] 0.5 + lut[u8(map1 scale1)]
// 0.5) w0 with both maps (save_image), lut[u8(map0 scale0)] w0 with map0 alone (save_labels), nothing with neither.
// w1 is not used and must be 0.  lut [256][3] u8 (NULL only without a layer).
extern "C" int avt_render_overlay(const float* img, int N, int H, int W, const float* map0, float scale0, double w0,
                                  const float* map1, float scale1, double w1, float wimg, const unsigned char* lut,
                                  unsigned char* out, void* stream) {
  AVT_REQUIRE(img && out, "render_overlay: null pointer");
  AVT_REQUIRE(N >= 1 && H >= 1 && W >= 1 && 3LL * H * W <= 0x7fffffffLL, "render_overlay: bad shape N=%d H=%d W=%d", N,
              H, W);
  AVT_REQUIRE(map0 || !map1, "render_overlay: map1 without map0");
  AVT_REQUIRE(lut || !map0, "render_overlay: a layer needs a colour table");
  AVT_REQUIRE(w1 == 0.0, "render_overlay: w1 is not used and must be 0");
  OverlayArgs a;
  a.img = img, a.map0 = map0, a.map1 = map1, a.lut = lut, a.out = out;
  a.HW = H * W;
  a.scale0 = scale0, a.scale1 = scale1, a.wimg = wimg, a.w0 = w0;
  const uintptr_t bits = (uintptr_t)img | (uintptr_t)map0 | (uintptr_t)map1;
  a.vec_in = (a.HW % 4 == 0) && (bits & 15u) == 0;
  hipStream_t st = (hipStream_t)stream;
  if (map1)
    hipLaunchKernelGGL(render_overlay_kernel<2>, dim3(N), dim3(RD_T), 0, st, a);
  else if (map0)
    hipLaunchKernelGGL(render_overlay_kernel<1>, dim3(N), dim3(RD_T), 0, st, a);
  else
    hipLaunchKernelGGL(render_overlay_kernel<0>, dim3(N), dim3(RD_T), 0, st, a);
  return check_launch("render_overlay");
}
