// Classifier head of the stand-alone R3D-18 (models/resnet3D.py:208-212 and the fine-tune loss of train_3D.py:89's
// recipe): AdaptiveAvgPool3d((1,1,1)) -> nn.Linear -> nn.CrossEntropyLoss with class labels, forward and backward.
//  * avt_cls_pool_fwd / _bwd   the average over the per = t*h*w positions of the layer4 map (bf16 [b][per][C]) and its
//                              broadcast backward.  The forward splits `per` into slots of kPoolRows rows, one block per
//                              (slot, clip, 512-channel tile); a slot's partial sums are written with plain stores and
//                              a second launch adds them in slot order (as the BatchNorm statistics do).  Both
//                              directions DIVIDE by (float)per (IEEE fp32 division; no reciprocal is formed).
//  * avt_cls_fc_fwd / _bwd     fp32 nn.Linear on the [b][C] features: one wave per output, lanes strided over C, the
//                              xor-butterfly wave sum; the backward's sums over b and n run sequentially in index order.
//  * avt_softmax_ce            mean CE over the valid rows (labels outside [0, n) are ignored rows), its gradient and
//                              the top-1 count; one block, one wave per row, rows and waves summed in index order.
// No atomics anywhere: identical inputs give identical bits.
#include "avt_common.h"
#include <math.h>

namespace avt {

constexpr int kPoolRows = 64;    // rows of one partial slot
constexpr int kPoolTileC = 512;  // channels of one block: 64 column groups of 8 x 4 row lanes = 256 threads

static inline long long pool_slots(long long per) { return (per + kPoolRows - 1) / kPoolRows; }

// ws[b][slot][C] = sum over the slot's rows of v[b][row][c]: thread (cg, rl) adds rows rl, rl+4, ... of column group
// cg, then the 4 row lanes are added in lane order through LDS
__global__ __launch_bounds__(256) void cls_pool_partial_kernel(const bf16_t* __restrict__ v, float* __restrict__ ws,
                                                               long long per, int C, int slots) {
  __shared__ float red[4][64][8];
  const int cg = threadIdx.x & 63, rl = threadIdx.x >> 6;
  const int slot = blockIdx.x, b = blockIdx.y;
  const int c0 = blockIdx.z * kPoolTileC + cg * 8;
  const long long r0 = (long long)slot * kPoolRows;
  const long long r1 = r0 + kPoolRows < per ? r0 + kPoolRows : per;
  float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  if (c0 < C) {
    const bf16_t* base = v + ((size_t)b * per) * C + c0;
    for (long long r = r0 + rl; r < r1; r += 4) {
      const u32x4 q = *reinterpret_cast<const u32x4*>(base + (size_t)r * C);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        acc[2 * e] += __uint_as_float(q[e] << 16);
        acc[2 * e + 1] += __uint_as_float(q[e] & 0xffff0000u);
      }
    }
  }
#pragma unroll
  for (int e = 0; e < 8; ++e) red[rl][cg][e] = acc[e];
  __syncthreads();
  if (rl == 0 && c0 < C) {
    float* out = ws + ((size_t)b * slots + slot) * C + c0;
#pragma unroll
    for (int e = 0; e < 8; ++e) out[e] = ((red[0][cg][e] + red[1][cg][e]) + red[2][cg][e]) + red[3][cg][e];
  }
}

// feat[b][c] = (sum of the slots, in slot order) / per
__global__ __launch_bounds__(256) void cls_pool_finish_kernel(const float* __restrict__ ws, float* __restrict__ feat,
                                                              int b, int C, int slots, float per) {
  const long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x;
  if (i >= (long long)b * C) return;
  const int bi = (int)(i / C), c = (int)(i % C);
  const float* p = ws + (size_t)bi * slots * C + c;
  float s = 0.f;
  for (int k = 0; k < slots; ++k) s += p[(size_t)k * C];
  feat[i] = s / per;
}

// g[b][row][c] = bf16(gfeat[b][c] / per) for every row: one 16-byte store per 8 channels
__global__ __launch_bounds__(256) void cls_pool_bwd_kernel(const float* __restrict__ gfeat, bf16_t* __restrict__ g,
                                                           long long per, int C, float perf) {
  const int cg8 = C / 8;
  const int b = blockIdx.y;
  const long long nvec = per * cg8;  // 16-byte vectors of this clip
  const float* gf = gfeat + (size_t)b * C;
  u32x4* out = reinterpret_cast<u32x4*>(g + (size_t)b * per * C);
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < nvec; i += (long long)gridDim.x * blockDim.x) {
    const int c = (int)(i % cg8) * 8;
    u32x4 q;
#pragma unroll
    for (int e = 0; e < 4; ++e) q[e] = pack2(gf[c + 2 * e] / perf, gf[c + 2 * e + 1] / perf);
    out[i] = q;
  }
}

// logits[b][n] = bias[n] + sum_c feat[b][c] * W[n][c]: one wave per n, every clip in turn
__global__ __launch_bounds__(256) void cls_fc_fwd_kernel(const float* __restrict__ feat, const float* __restrict__ W,
                                                         const float* __restrict__ bias, float* __restrict__ logits,
                                                         int b, int C, int n) {
  const int lane = threadIdx.x & 63;
  const int j = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (j >= n) return;  // whole waves leave together
  const float* w = W + (size_t)j * C;
  const float bj = bias[j];
  for (int i = 0; i < b; ++i) {
    const float* f = feat + (size_t)i * C;
    float s = 0.f;
    for (int c = lane; c < C; c += 64) s += f[c] * w[c];
    s = wave_sum(s);
    if (lane == 0) logits[(size_t)i * n + j] = bj + s;
  }
}

// gW[j][c] = sum_i dl[i][j] * feat[i][c] (i increasing); gbias[j] = sum_i dl[i][j]: one thread per (j, c)
__global__ __launch_bounds__(256) void cls_fc_wgrad_kernel(const float* __restrict__ dl, const float* __restrict__ feat,
                                                           float* __restrict__ gW, float* __restrict__ gbias, int b,
                                                           int C, int n) {
  const long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x;
  if (i >= (long long)n * C) return;
  const int j = (int)(i / C), c = (int)(i % C);
  float s = 0.f, sb = 0.f;
  for (int k = 0; k < b; ++k) {
    const float d = dl[(size_t)k * n + j];
    s += d * feat[(size_t)k * C + c];
    sb += d;
  }
  gW[i] = s;
  if (c == 0) gbias[j] = sb;
}

// gfeat[i][c] = sum_j dl[i][j] * W[j][c] (j increasing): one thread per (i, c)
__global__ __launch_bounds__(256) void cls_fc_dgrad_kernel(const float* __restrict__ dl, const float* __restrict__ W,
                                                           float* __restrict__ gfeat, int b, int C, int n) {
  const long long t = blockIdx.x * (long long)blockDim.x + threadIdx.x;
  if (t >= (long long)b * C) return;
  const int i = (int)(t / C), c = (int)(t % C);
  const float* d = dl + (size_t)i * n;
  float s = 0.f;
  for (int j = 0; j < n; ++j) s += d[j] * W[(size_t)j * C + c];
  gfeat[t] = s;
}

__device__ __forceinline__ int wave_sum_int(int v) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// One block of 1024 threads: wave w takes rows w, w+16, ..., its lanes strided over the n logits (any n: the strided
// passes of hardway_ce_kernel's wide-row loop).  A row whose label lies outside [0, n) is ignored: no loss, a +0
// gradient row, not counted in the denominator.  No valid row: loss 0, every gradient +0.
__global__ __launch_bounds__(1024) void softmax_ce_kernel(const float* __restrict__ z, const long long* __restrict__ labels,
                                                          int B, int n, float scale, float* __restrict__ loss,
                                                          float* __restrict__ dz, int* __restrict__ correct) {
  __shared__ float red[16];
  __shared__ int redi[16], redc[16];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  int cnt = 0;
  for (int i = threadIdx.x; i < B; i += 1024) {
    const long long y = labels[i];
    cnt += (y >= 0 && y < n) ? 1 : 0;
  }
  cnt = wave_sum_int(cnt);
  if (lane == 0) redi[w] = cnt;
  __syncthreads();
  int nvalid = 0;
  for (int k = 0; k < 16; ++k) nvalid += redi[k];
  const float fvalid = (float)nvalid;
  float part = 0.f;
  int hit = 0;
  for (int i = w; i < B; i += 16) {
    const long long y = labels[i];
    const float* r = z + (size_t)i * n;
    if (!(y >= 0 && y < n)) {
      if (dz)
        for (int j = lane; j < n; j += 64) dz[(size_t)i * n + j] = 0.f;
      continue;
    }
    float mx = -INFINITY;
    int am = 0x7fffffff;
    for (int j = lane; j < n; j += 64) {
      const float x = r[j];
      if (x > mx || am == 0x7fffffff) {  // the first index a lane sees, then strictly larger values only
        mx = x;
        am = j;
      }
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
      const float ox = __shfl_xor(mx, o, 64);
      const int oa = __shfl_xor(am, o, 64);
      if (oa != 0x7fffffff && (am == 0x7fffffff || ox > mx || (ox == mx && oa < am))) {
        mx = ox;
        am = oa;
      }
    }
    float se = 0.f;
    for (int j = lane; j < n; j += 64) se += expf(r[j] - mx);
    se = wave_sum(se);
    const float lse = mx + logf(se);
    if (lane == 0) {
      part += lse - r[y];
      hit += (am == (int)y) ? 1 : 0;
    }
    if (dz) {
      for (int j = lane; j < n; j += 64)
        dz[(size_t)i * n + j] = (expf(r[j] - lse) - (j == (int)y ? 1.f : 0.f)) * scale / fvalid;
    }
  }
  if (lane == 0) {
    red[w] = part;
    redc[w] = hit;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    float t = 0.f;
    int h = 0;
    for (int k = 0; k < 16; ++k) {
      t += red[k];
      h += redc[k];
    }
    loss[0] = nvalid > 0 ? t * scale / fvalid : 0.f;
    if (correct) correct[0] = h;
  }
}

}  // namespace avt

using namespace avt;

static bool pool_shape_ok(int b, long long per, int C) {
  // per < 2^24: (float)per is exact; b and the channel tiles are grid dimensions
  return b >= 1 && b <= 65535 && per >= 1 && per < (1ll << 24) && C >= 8 && C % 8 == 0 && C <= 65535 * 8;
}

extern "C" size_t avt_cls_pool_ws_bytes(int b, long long per, int C) {
  if (!pool_shape_ok(b, per, C)) return 0;
  return (size_t)b * (size_t)pool_slots(per) * (size_t)C * sizeof(float);
}

extern "C" int avt_cls_pool_fwd(const void* v, float* feat, int b, long long per, int C, void* workspace,
                                size_t ws_bytes, void* stream) {
  AVT_REQUIRE(v && feat, "cls_pool_fwd: null pointer");
  AVT_REQUIRE(pool_shape_ok(b, per, C), "cls_pool_fwd: need b >= 1, 1 <= per < 2^24, C %% 8 == 0 (b=%d per=%lld C=%d)",
              b, per, C);
  AVT_REQUIRE((uintptr_t)v % 16 == 0, "cls_pool_fwd: v must be 16-byte aligned");
  const size_t need = avt_cls_pool_ws_bytes(b, per, C);
  AVT_REQUIRE(workspace && ws_bytes >= need, "cls_pool_fwd: workspace of %zu bytes needed (avt_cls_pool_ws_bytes), got %zu",
              need, workspace ? ws_bytes : (size_t)0);
  const int slots = (int)pool_slots(per);
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid(slots, b, (C + kPoolTileC - 1) / kPoolTileC);
  hipLaunchKernelGGL(cls_pool_partial_kernel, grid, dim3(256), 0, st, (const bf16_t*)v, (float*)workspace, per, C, slots);
  const long long nout = (long long)b * C;
  hipLaunchKernelGGL(cls_pool_finish_kernel, dim3((unsigned)((nout + 255) / 256)), dim3(256), 0, st,
                     (const float*)workspace, feat, b, C, slots, (float)per);
  return check_launch("cls_pool_fwd");
}

extern "C" int avt_cls_pool_bwd(const float* gfeat, void* g, int b, long long per, int C, void* stream) {
  AVT_REQUIRE(gfeat && g, "cls_pool_bwd: null pointer");
  AVT_REQUIRE(pool_shape_ok(b, per, C), "cls_pool_bwd: need b >= 1, 1 <= per < 2^24, C %% 8 == 0 (b=%d per=%lld C=%d)",
              b, per, C);
  AVT_REQUIRE((uintptr_t)g % 16 == 0, "cls_pool_bwd: g must be 16-byte aligned");
  const long long nvec = per * (C / 8);
  long long blocks = (nvec + 255) / 256;
  if (blocks > 1024) blocks = 1024;
  hipLaunchKernelGGL(cls_pool_bwd_kernel, dim3((unsigned)blocks, b), dim3(256), 0, (hipStream_t)stream, gfeat,
                     (bf16_t*)g, per, C, (float)per);
  return check_launch("cls_pool_bwd");
}

static bool fc_shape_ok(int b, int C, int n) {
  return b >= 1 && C >= 1 && n >= 1 && (long long)n * C < (1ll << 31) && (long long)b * C < (1ll << 31) &&
         (long long)b * n < (1ll << 31);
}

extern "C" int avt_cls_fc_fwd(const float* feat, const float* W, const float* bias, float* logits, int b, int C, int n,
                              void* stream) {
  AVT_REQUIRE(feat && W && bias && logits, "cls_fc_fwd: null pointer");
  AVT_REQUIRE(fc_shape_ok(b, C, n), "cls_fc_fwd: bad shape (b=%d C=%d n=%d)", b, C, n);
  hipLaunchKernelGGL(cls_fc_fwd_kernel, dim3((n + 3) / 4), dim3(256), 0, (hipStream_t)stream, feat, W, bias, logits, b,
                     C, n);
  return check_launch("cls_fc_fwd");
}

extern "C" int avt_cls_fc_bwd(const float* dlogits, const float* feat, const float* W, float* gW, float* gbias,
                              float* gfeat, int b, int C, int n, void* stream) {
  AVT_REQUIRE(dlogits && feat && W && gW && gbias && gfeat, "cls_fc_bwd: null pointer");
  AVT_REQUIRE(fc_shape_ok(b, C, n), "cls_fc_bwd: bad shape (b=%d C=%d n=%d)", b, C, n);
  hipStream_t st = (hipStream_t)stream;
  const long long nw = (long long)n * C, nf = (long long)b * C;
  hipLaunchKernelGGL(cls_fc_wgrad_kernel, dim3((unsigned)((nw + 255) / 256)), dim3(256), 0, st, dlogits, feat, gW, gbias,
                     b, C, n);
  hipLaunchKernelGGL(cls_fc_dgrad_kernel, dim3((unsigned)((nf + 255) / 256)), dim3(256), 0, st, dlogits, W, gfeat, b, C,
                     n);
  return check_launch("cls_fc_bwd");
}

extern "C" int avt_softmax_ce(const float* logits, const long long* labels, int b, int n, float scale, float* loss,
                              float* dlogits, int* correct, void* stream) {
  AVT_REQUIRE(logits && labels && loss, "softmax_ce: null pointer");
  AVT_REQUIRE(b >= 1 && n >= 1 && (long long)b * n < (1ll << 31), "softmax_ce: bad shape (b=%d n=%d)", b, n);
  AVT_REQUIRE((uintptr_t)labels % 8 == 0, "softmax_ce: labels must be 8-byte aligned int64");
  hipLaunchKernelGGL(softmax_ce_kernel, dim3(1), dim3(1024), 0, (hipStream_t)stream, logits, labels, b, n, scale, loss,
                     dlogits, correct);
  return check_launch("softmax_ce");
}
