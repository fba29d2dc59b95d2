// Flow-compensated temporal consistency (flow.py:133-157 of the reference, downstream of "a flow field exists"):
// the bilinear warp of a map by a field, the consistency cIoU of consecutive binary maps under it, the trainable L1
// form of the same at heat-map resolution, and the Middlebury colour picture of a field (utils.py:64-192).
//
// One sampling definition, bilinear_at, serves the first three.  Every product and sum in it is a separately
// rounded fp32 operation (exact_fp.h), so the numpy float32 restatement (tests/flow_oracle.py) reproduces it bit
// for bit; the consistency sums are integer counts, the colour chain is fp64 with separately rounded operations as
// numpy evaluates it.  No float atomics: the same inputs give the same bytes.
//
// Block shapes.  These kernels have no arithmetic to speak of: one 8-byte field load, four
// gathered map reads and a handful of VALU operations per pixel, so what matters is having waves on many CUs.
//  * warp: one thread per output pixel, 256-thread blocks, grid (ceil(Ho Wo / 256), min(N, 65535)), maps beyond the
//    y limit by a stride loop.  Consecutive lanes load consecutive 8-byte field entries (512 B per wave instruction).
//  * consistency, colour: (chunks, maps) blocks of 256 threads, chunks = clamp(ceil(pixels / 2048), 1, 64), each block
//    walking its map with stride chunks * 256.  One block per pair, as pair_ciou_kernel has it, would put a video's
//    15 pairs on 15 of the 256 CUs with 49 dependent gather rounds per thread at 224 x 224; in chunks the same video
//    is 375 blocks (1.5 per CU, 8 rounds each).  The per-chunk results (three counts / one maximum) go to a workspace
//    and a second launch (consistency) or the head of the second launch (colour) combines them; counts and maxima
//    are exact in any order.
//  * loss: one block per (clip, frame), 256 threads: it evaluates its frame's pair once into LDS (sign, four weights,
//    four cell indices per output pixel: 28 KiB at the 1024-pixel limit), then every thread gathers over all output
//    pixels for the source pixels it owns.  In the gather all lanes read the same LDS entry (a broadcast: no bank
//    conflict), 16 + 8 + 4 bytes wide.
#include "avt_common.h"
#include "exact_fp.h"

namespace avt {

constexpr int FL_T = 256;
constexpr int FL_CHUNK_PIXELS = 2048;
constexpr int FL_MAX_CHUNKS = 64;
constexpr int FL_LOSS_MAXP = 1024;
constexpr int FL_NCOLS = 55;

static inline int flow_chunks(long long pixels) {
  long long c = (pixels + FL_CHUNK_PIXELS - 1) / FL_CHUNK_PIXELS;
  return (int)(c < 1 ? 1 : (c > FL_MAX_CHUNKS ? FL_MAX_CHUNKS : c));
}

__device__ __forceinline__ float map_at(const float* m, int i) { return m[i]; }
__device__ __forceinline__ float map_at(const unsigned char* m, int i) { return m[i] ? 1.f : 0.f; }

// Sampling position of output pixel (x, y) from its field entry (fx, fy): coords 0, grid_sample's un-normalisation
// for align_corners=False, ((g + 1) * size - 1) / 2; coords 1, pixel displacements, x + u.
__device__ __forceinline__ void flow_position(int coords, float fx, float fy, int x, int y, int W, int H, float& ix,
                                              float& iy) {
  if (coords == 0) {
    ix = div_rn(sub_rn(mul_rn(add_rn(fx, 1.f), (float)W), 1.f), 2.f);
    iy = div_rn(sub_rn(mul_rn(add_rn(fy, 1.f), (float)H), 1.f), 2.f);
  } else {
    ix = add_rn((float)x, fx);
    iy = add_rn((float)y, fy);
  }
}

// The four neighbours of a sampling position: cell index y * W + x of each (-1 outside the map) and its weight, in the
// order nw, ne, sw, se.  A non-finite position has no neighbour.  The floor is clamped to [-2, size + 1] before the int
// conversion (every clamped value is outside the map on both neighbours, as the unclamped one is).
struct Taps {
  int cell[4];
  float w[4];
};

__device__ __forceinline__ Taps flow_taps(int H, int W, float ix, float iy) {
  Taps t;
  if (!(fabsf(ix) < INFINITY) || !(fabsf(iy) < INFINITY)) {  // NaN or +-inf
    for (int c = 0; c < 4; ++c) {
      t.cell[c] = -1;
      t.w[c] = 0.f;
    }
    return t;
  }
  const float fx0 = floorf(ix), fy0 = floorf(iy);
  const float wx1 = sub_rn(ix, fx0), wy1 = sub_rn(iy, fy0);                          // ix - x0, iy - y0
  const float wx0 = sub_rn(add_rn(fx0, 1.f), ix), wy0 = sub_rn(add_rn(fy0, 1.f), iy);  // x0 + 1 - ix, y0 + 1 - iy
  const int x0 = (int)fminf(fmaxf(fx0, -2.f), (float)W + 1.f);
  const int y0 = (int)fminf(fmaxf(fy0, -2.f), (float)H + 1.f);
  const bool xin0 = x0 >= 0 && x0 < W, xin1 = x0 + 1 >= 0 && x0 + 1 < W;
  const bool yin0 = y0 >= 0 && y0 < H, yin1 = y0 + 1 >= 0 && y0 + 1 < H;
  t.w[0] = mul_rn(wx0, wy0);
  t.w[1] = mul_rn(wx1, wy0);
  t.w[2] = mul_rn(wx0, wy1);
  t.w[3] = mul_rn(wx1, wy1);
  t.cell[0] = xin0 && yin0 ? y0 * W + x0 : -1;
  t.cell[1] = xin1 && yin0 ? y0 * W + x0 + 1 : -1;
  t.cell[2] = xin0 && yin1 ? (y0 + 1) * W + x0 : -1;
  t.cell[3] = xin1 && yin1 ? (y0 + 1) * W + x0 + 1 : -1;
  return t;
}

// nw*m[y0][x0] + ne*m[y0][x0+1] + sw*m[y0+1][x0] + se*m[y0+1][x0+1], the terms added in that order starting from the
// first one inside the map; outside neighbours contribute nothing; no neighbour at all gives +0.
template <typename T>
__device__ __forceinline__ float taps_sum(const T* __restrict__ m, const Taps& t) {
  float acc = 0.f;
  bool any = false;
#pragma unroll
  for (int c = 0; c < 4; ++c)
    if (t.cell[c] >= 0) {
      const float term = mul_rn(t.w[c], map_at(m, t.cell[c]));
      acc = any ? add_rn(acc, term) : term;
      any = true;
    }
  return acc;
}

template <typename T>
__device__ __forceinline__ float bilinear_at(const T* __restrict__ m, int H, int W, float ix, float iy) {
  return taps_sum(m, flow_taps(H, W, ix, iy));
}

// ---- warp ----
template <typename T>
__global__ __launch_bounds__(FL_T) void flow_warp_kernel(const T* __restrict__ src, int N, int H, int W,
                                                         const float2* __restrict__ field, int Ho, int Wo, int coords,
                                                         float* __restrict__ out) {
  const int P = Ho * Wo;
  const int i = blockIdx.x * FL_T + threadIdx.x;
  if (i >= P) return;
  const int y = i / Wo, x = i - y * Wo;
  for (int n = blockIdx.y; n < N; n += gridDim.y) {
    const float2 g = field[(size_t)n * P + i];
    float ix, iy;
    flow_position(coords, g.x, g.y, x, y, W, H, ix, iy);
    out[(size_t)n * P + i] = bilinear_at(src + (size_t)n * H * W, H, W, ix, iy);
  }
}

// ---- consistency: per-chunk counts, then one wave per pair ----
__global__ __launch_bounds__(FL_T) void flow_consistency_kernel(const unsigned char* __restrict__ pred,
                                                                const float2* __restrict__ field, int S, int coords,
                                                                unsigned* __restrict__ ws) {
  __shared__ unsigned red[3][FL_T / 64];
  const int k = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int n = S * S;
  const unsigned char* a = pred + (size_t)k * n;
  const unsigned char* b = a + n;
  const float2* f = field + (size_t)k * n;
  unsigned s_ig = 0, s_g = 0, s_i0 = 0;
  for (int i = blockIdx.x * FL_T + tid; i < n; i += gridDim.x * FL_T) {
    const int y = i / S, x = i - y * S;
    const float2 g = f[i];
    float ix, iy;
    flow_position(coords, g.x, g.y, x, y, S, S, ix, iy);
    const unsigned inf = bilinear_at(a, S, S, ix, iy) >= 0.5f ? 1u : 0u;
    const unsigned gv = b[i] ? 1u : 0u;
    s_ig += inf & gv;
    s_g += gv;
    s_i0 += inf & (gv ^ 1u);
  }
  for (int o = 32; o >= 1; o >>= 1) {
    s_ig += __shfl_xor(s_ig, o, 64);
    s_g += __shfl_xor(s_g, o, 64);
    s_i0 += __shfl_xor(s_i0, o, 64);
  }
  if (lane == 0) {
    red[0][wv] = s_ig;
    red[1][wv] = s_g;
    red[2][wv] = s_i0;
  }
  __syncthreads();
  if (tid < 3) {
    unsigned t = 0;
    for (int j = 0; j < FL_T / 64; ++j) t += red[tid][j];
    ws[((size_t)k * gridDim.x + blockIdx.x) * 3 + tid] = t;
  }
}

// out[k] = (inter / denom, inter, denom), denom = sum gt + sum infer * (gt == 0)   (utils.py:209-214)
__global__ __launch_bounds__(64) void flow_consistency_finish_kernel(const unsigned* __restrict__ ws, int chunks,
                                                                     double* __restrict__ out) {
  const int k = blockIdx.x, lane = threadIdx.x;
  unsigned long long v[3] = {0, 0, 0};
  if (lane < chunks)
    for (int j = 0; j < 3; ++j) v[j] = ws[((size_t)k * chunks + lane) * 3 + j];
  for (int o = 32; o >= 1; o >>= 1)
    for (int j = 0; j < 3; ++j) v[j] += __shfl_xor(v[j], o, 64);
  if (lane == 0) {
    const double inter = (double)v[0], denom = (double)v[1] + (double)v[2];
    out[k * 3 + 0] = inter / denom;
    out[k * 3 + 1] = inter;
    out[k * 3 + 2] = denom;
  }
}

// ---- loss ----
__device__ __forceinline__ float sgn3(float v) { return v > 0.f ? 1.f : (v < 0.f ? -1.f : 0.f); }

// Block (clip c, frame s) of x [b][t][P = h w].  With d_s(p) = bilinear_at(x[c, s])(p) - x[c, s+1](p):
//   s < t-1: ws[c (t-1) + s] = sum_p |d_s(p)| (per-thread sums over p = tid, tid + 256, ..., then block_sum's order)
//   dx[c, s, q] = (+0  +  kinv * sum_p sum_corner sign(d_s(p)) * weight(p, corner -> q))  -  sign(d_{s-1}(q)) * kinv
// the gather running over p increasing and the corners nw, ne, sw, se, the first bracket present for s < t-1 and
// the last term for s > 0; every operation separately rounded.
__global__ __launch_bounds__(FL_T) void flow_loss_kernel(const float* __restrict__ x, const float2* __restrict__ field,
                                                         int t, int h, int w, int coords, float kinv,
                                                         float* __restrict__ dx, float* __restrict__ ws) {
  __shared__ float4 s_w[FL_LOSS_MAXP];
  __shared__ short4 s_cell[FL_LOSS_MAXP];
  __shared__ float s_sgn[FL_LOSS_MAXP];
  __shared__ float red[FL_T / 64];
  const int P = h * w, tid = threadIdx.x;
  const int c = blockIdx.x / t, s = blockIdx.x - c * t;
  const float* xs = x + (size_t)blockIdx.x * P;
  if (s + 1 < t) {
    const float2* f = field + ((size_t)c * (t - 1) + s) * P;
    float a = 0.f;
    for (int p = tid; p < P; p += FL_T) {
      const int y = p / w, xx = p - y * w;
      const float2 g = f[p];
      float ix, iy;
      flow_position(coords, g.x, g.y, xx, y, w, h, ix, iy);
      const Taps tp = flow_taps(h, w, ix, iy);
      const float d = sub_rn(taps_sum(xs, tp), xs[P + p]);
      a = add_rn(a, fabsf(d));
      s_sgn[p] = sgn3(d);
      s_w[p] = make_float4(tp.w[0], tp.w[1], tp.w[2], tp.w[3]);
      s_cell[p] = make_short4((short)tp.cell[0], (short)tp.cell[1], (short)tp.cell[2], (short)tp.cell[3]);
    }
    a = block_sum(a, red);  // its barriers also publish the LDS tables
    if (tid == 0) ws[(size_t)c * (t - 1) + s] = a;
  }
  if (!dx) return;
  for (int q = tid; q < P; q += FL_T) {
    float g = 0.f;
    if (s + 1 < t) {
      float acc = 0.f;
      for (int p = 0; p < P; ++p) {
        const short4 cell = s_cell[p];
        const float4 wt = s_w[p];
        const float sg = s_sgn[p];
        if (cell.x == q) acc = add_rn(acc, mul_rn(sg, wt.x));
        if (cell.y == q) acc = add_rn(acc, mul_rn(sg, wt.y));
        if (cell.z == q) acc = add_rn(acc, mul_rn(sg, wt.z));
        if (cell.w == q) acc = add_rn(acc, mul_rn(sg, wt.w));
      }
      g = add_rn(g, mul_rn(acc, kinv));
    }
    if (s > 0) {
      const int y = q / w, xx = q - y * w;
      const float2 gp = field[((size_t)c * (t - 1) + s - 1) * P + q];
      float ix, iy;
      flow_position(coords, gp.x, gp.y, xx, y, w, h, ix, iy);
      const float d = sub_rn(bilinear_at(xs - P, h, w, ix, iy), xs[q]);
      g = sub_rn(g, mul_rn(sgn3(d), kinv));
    }
    dx[(size_t)blockIdx.x * P + q] = g;
  }
}

// loss = kinv * sum_{i < n} ws[i]: per-thread sums over i = tid, tid + 256, ..., then block_sum's order
__global__ __launch_bounds__(FL_T) void flow_loss_finish_kernel(const float* __restrict__ ws, int n, float kinv,
                                                                float* __restrict__ loss) {
  __shared__ float red[FL_T / 64];
  float a = 0.f;
  for (int i = threadIdx.x; i < n; i += FL_T) a = add_rn(a, ws[i]);
  a = block_sum(a, red);
  if (threadIdx.x == 0) *loss = mul_rn(a, kinv);
}

// ---- colour ----
// utils.flow2img's first half per pixel: components beyond 1e7 mark the pixel unknown and are zeroed
__device__ __forceinline__ bool flow_known(float2 g, double& u, double& v) {
  u = (double)g.x;
  v = (double)g.y;
  const bool unknown = fabs(u) > 1e7 || fabs(v) > 1e7;
  if (unknown) u = v = 0.0;
  return !unknown;
}

__device__ __forceinline__ double flow_rad(double u, double v) {
  return sqrt(add_rn(mul_rn(u, u), mul_rn(v, v)));
}

// ws[n][chunk] = max over the chunk's pixels of sqrt(u^2 + v^2), started at -1 (flow2img's max(-1, .)); a NaN radius
// does not take part
__global__ __launch_bounds__(FL_T) void flow_maxrad_kernel(const float2* __restrict__ field, int P,
                                                           double* __restrict__ ws) {
  __shared__ double red[FL_T / 64];
  const int n = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const float2* f = field + (size_t)n * P;
  double m = -1.0;
  for (int i = blockIdx.x * FL_T + tid; i < P; i += gridDim.x * FL_T) {
    double u, v;
    flow_known(f[i], u, v);
    m = fmax(m, flow_rad(u, v));
  }
  for (int o = 32; o >= 1; o >>= 1) m = fmax(m, __shfl_xor(m, o, 64));
  if (lane == 0) red[wv] = m;
  __syncthreads();
  if (tid == 0) {
    for (int j = 1; j < FL_T / 64; ++j) m = fmax(m, red[j]);
    ws[(size_t)n * gridDim.x + blockIdx.x] = m;
  }
}

__global__ __launch_bounds__(FL_T) void flow_color_kernel(const float2* __restrict__ field, int P,
                                                          const double* __restrict__ ws,
                                                          const unsigned char* __restrict__ wheel,
                                                          unsigned char* __restrict__ out) {
  __shared__ double s_wheel[FL_NCOLS * 3];  // wheel / 255
  __shared__ double s_max;
  const int n = blockIdx.y, tid = threadIdx.x;
  if (tid < FL_NCOLS * 3) s_wheel[tid] = div_rn((double)wheel[tid], 255.0);
  if (tid == 0) {
    double m = -1.0;
    for (int j = 0; j < (int)gridDim.x; ++j) m = fmax(m, ws[(size_t)n * gridDim.x + j]);
    s_max = m;
  }
  __syncthreads();
  const double maxrad = s_max;
  const double eps = 2.220446049250313e-16, pi = 3.141592653589793;
  const float2* f = field + (size_t)n * P;
  unsigned char* o = out + (size_t)n * P * 3;
  for (int i = blockIdx.x * FL_T + tid; i < P; i += gridDim.x * FL_T) {
    double u, v;
    const bool known = flow_known(f[i], u, v);
    u = add_rn(div_rn(u, maxrad), eps);
    v = add_rn(div_rn(v, maxrad), eps);
    const bool isnan_uv = (u != u) || (v != v);  // compute_color's NAN_idx
    if (isnan_uv) u = v = 0.0;
    const double rad = flow_rad(u, v);
    const double a = div_rn(atan2(-v, -u), pi);
    const double fk = add_rn(mul_rn(div_rn(add_rn(a, 1.0), 2.0), (double)(FL_NCOLS - 1)), 1.0);
    const double fk0 = floor(fk);
    int k0 = (int)fk0;
    k0 = k0 < 1 ? 1 : (k0 > FL_NCOLS ? FL_NCOLS : k0);  // a in [-1, 1] gives 1 .. 55; the clamp guards the table
    int k1 = k0 + 1;
    if (k1 == FL_NCOLS + 1) k1 = 1;
    const double fr = sub_rn(fk, fk0);
    for (int ch = 0; ch < 3; ++ch) {
      const double col0 = s_wheel[(k0 - 1) * 3 + ch], col1 = s_wheel[(k1 - 1) * 3 + ch];
      double col = add_rn(mul_rn(sub_rn(1.0, fr), col0), mul_rn(fr, col1));
      if (rad <= 1.0)
        col = sub_rn(1.0, mul_rn(rad, sub_rn(1.0, col)));
      else
        col = mul_rn(col, 0.75);
      const double b = floor(mul_rn(mul_rn(255.0, col), isnan_uv ? 0.0 : 1.0));
      o[(size_t)i * 3 + ch] = known ? (unsigned char)fmin(fmax(b, 0.0), 255.0) : (unsigned char)0;
    }
  }
}

}  // namespace avt

using namespace avt;

// a map of a x b pixels whose flat pixel index, plus a block's overshoot, stays an int
static bool flow_dims_ok(long long a, long long b) { return a >= 1 && b >= 1 && a * b <= (1LL << 30); }

extern "C" size_t avt_flow_workspace_bytes(int maps, long long pixels) {
  if (maps < 1 || pixels < 1) return 0;
  return (size_t)maps * (size_t)flow_chunks(pixels) * 16;
}

extern "C" int avt_flow_warp(const void* src, int src_u8, int N, int H, int W, const float* field, int Ho, int Wo,
                             int coords, float* out, void* stream) {
  AVT_REQUIRE(src && field && out, "flow_warp: null pointer");
  AVT_REQUIRE(N >= 1 && flow_dims_ok(H, W) && flow_dims_ok(Ho, Wo),
              "flow_warp: bad shape N=%d H=%d W=%d Ho=%d Wo=%d (sizes >= 1, H*W and Ho*Wo <= 2^30)", N, H, W, Ho, Wo);
  AVT_REQUIRE(coords == 0 || coords == 1, "flow_warp: coords must be 0 (grid) or 1 (pixels), got %d", coords);
  AVT_REQUIRE(src_u8 == 0 || src_u8 == 1, "flow_warp: src_u8 must be 0 (fp32) or 1 (u8), got %d", src_u8);
  AVT_REQUIRE(coords == 0 || (Ho == H && Wo == W), "flow_warp: pixel displacements need a field of the map's size "
              "(H=%d W=%d Ho=%d Wo=%d)", H, W, Ho, Wo);
  AVT_REQUIRE(((uintptr_t)field & 7) == 0, "flow_warp: field must be 8-byte aligned (both components are one load)");
  AVT_REQUIRE(((uintptr_t)out & 3) == 0 && (src_u8 || ((uintptr_t)src & 3) == 0), "flow_warp: misaligned pointer");
  const dim3 grid((Ho * Wo + FL_T - 1) / FL_T, N < 65535 ? N : 65535);
  hipStream_t st = (hipStream_t)stream;
  if (src_u8)
    hipLaunchKernelGGL(flow_warp_kernel<unsigned char>, grid, dim3(FL_T), 0, st, (const unsigned char*)src, N, H, W,
                       (const float2*)field, Ho, Wo, coords, out);
  else
    hipLaunchKernelGGL(flow_warp_kernel<float>, grid, dim3(FL_T), 0, st, (const float*)src, N, H, W,
                       (const float2*)field, Ho, Wo, coords, out);
  return check_launch("flow_warp");
}

extern "C" int avt_flow_consistency(const void* pred, int T, int S, const float* field, int coords, double* out,
                                    void* workspace, void* stream) {
  AVT_REQUIRE(pred && field && out && workspace, "flow_consistency: null pointer");
  AVT_REQUIRE(T >= 2 && T <= 65536 && S >= 1 && S <= 32768,
              "flow_consistency: need 2 <= T <= 65536 maps of 1 <= S <= 32768 (T=%d S=%d)", T, S);
  AVT_REQUIRE(coords == 0 || coords == 1, "flow_consistency: coords must be 0 (grid) or 1 (pixels), got %d", coords);
  AVT_REQUIRE(((uintptr_t)field & 7) == 0 && ((uintptr_t)out & 7) == 0 && ((uintptr_t)workspace & 7) == 0,
              "flow_consistency: field, out and workspace must be 8-byte aligned");
  const int chunks = flow_chunks((long long)S * S);
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(flow_consistency_kernel, dim3(chunks, T - 1), dim3(FL_T), 0, st, (const unsigned char*)pred,
                     (const float2*)field, S, coords, (unsigned*)workspace);
  hipLaunchKernelGGL(flow_consistency_finish_kernel, dim3(T - 1), dim3(64), 0, st, (const unsigned*)workspace, chunks,
                     out);
  return check_launch("flow_consistency");
}

extern "C" int avt_flow_loss(const float* x, int b, int t, int h, int w, const float* field, int coords, float* loss,
                             float* dx, float* ws, void* stream) {
  AVT_REQUIRE(x && field && loss && ws, "flow_loss: null pointer");
  AVT_REQUIRE(b >= 1 && t >= 2 && h >= 1 && w >= 1 && (long long)b * t <= 0x7fffffffLL,
              "flow_loss: need b >= 1, t >= 2, h >= 1, w >= 1 (b=%d t=%d h=%d w=%d)", b, t, h, w);
  AVT_REQUIRE((long long)h * w <= FL_LOSS_MAXP, "flow_loss: h*w = %lld is above the %d pixels one block holds",
              (long long)h * w, FL_LOSS_MAXP);
  AVT_REQUIRE(coords == 0 || coords == 1, "flow_loss: coords must be 0 (grid) or 1 (pixels), got %d", coords);
  AVT_REQUIRE(((uintptr_t)field & 7) == 0, "flow_loss: field must be 8-byte aligned (both components are one load)");
  hipStream_t st = (hipStream_t)stream;
  const float kinv = 1.f / ((float)b * (float)(t - 1) * (float)(h * w));
  hipLaunchKernelGGL(flow_loss_kernel, dim3(b * t), dim3(FL_T), 0, st, x, (const float2*)field, t, h, w, coords, kinv,
                     dx, ws);
  hipLaunchKernelGGL(flow_loss_finish_kernel, dim3(1), dim3(FL_T), 0, st, ws, b * (t - 1), kinv, loss);
  return check_launch("flow_loss");
}

extern "C" int avt_flow_color(const float* field, int N, int H, int W, const unsigned char* wheel, unsigned char* out,
                              void* workspace, void* stream) {
  AVT_REQUIRE(field && wheel && out && workspace, "flow_color: null pointer");
  AVT_REQUIRE(N >= 1 && N <= 65535 && flow_dims_ok(H, W),
              "flow_color: bad shape N=%d H=%d W=%d (1 <= N <= 65535)", N, H, W);
  AVT_REQUIRE(((uintptr_t)field & 7) == 0 && ((uintptr_t)workspace & 7) == 0,
              "flow_color: field and workspace must be 8-byte aligned");
  const int P = H * W, chunks = flow_chunks(P);
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(flow_maxrad_kernel, dim3(chunks, N), dim3(FL_T), 0, st, (const float2*)field, P,
                     (double*)workspace);
  hipLaunchKernelGGL(flow_color_kernel, dim3(chunks, N), dim3(FL_T), 0, st, (const float2*)field, P,
                     (const double*)workspace, wheel, out);
  return check_launch("flow_color");
}
