/* libavt — MI355X (gfx950) C-ABI for the audio-visual hard-way train step.
 *
 * Every entry point takes plain device pointers + sizes and a hipStream_t (as void*), launches
 * asynchronously on that stream, never allocates, never synchronises the host, and returns
 * AVT_OK (0) or a negative code; avt_last_error() returns a thread-local message.
 * Buffers are owned by the caller (PyTorch's caching allocator in the Python host).
 *
 * Layouts: activations NHWC bf16 (raw uint16 bits); statistics/head fp32;
 * conv master weights fp32 in OHWI order (== channels_last OIHW parameters).
 *
 * Reference interface each entry point replaces (tonymisic/audio-visual-tubes):
 *   avt_conv2d_fwd/dgrad/wgrad   nn.Conv2d fwd + autograd bwd of conv3x3/conv1x1/stems
 *                                (models/base_models.py:23-30, 135-138; called at 53-69, 195-210)
 *   avt_bn_finalize/apply/bwd    nn.BatchNorm2d train mode + nn.ReLU(inplace) + residual add
 *                                (models/base_models.py:39, 46-49, 58-67, 120-121, 141)
 *   avt_maxpool3s2_fwd/bwd       nn.MaxPool2d(3, 2, 1) (models/base_models.py:143, 203)
 *   avt_stem_*                   stem bn1 -> relu -> maxpool fused fwd/bwd (models/base_models.py:200-203)
 *   avt_bn_relu_bwd              BasicBlock bn1+relu backward, mask from the pre-activation (base_models.py:47-48)
 *   avt_bn_apply_mask,           BasicBlock output relu(bn2(c2) + residual) (base_models.py:64-67) with its ReLU
 *   avt_bn_bwd_mask,             mask kept as bits; the backward of bn2 (+ downsample.1) from those bits, and the
 *   avt_conv2d_dgrad_mask        identity block's input gradient dgrad(conv1) + g * mask without a stored g'
 *   avt_bn_eval_bwd,             the same BatchNorm2d layers in eval mode (running statistics, nn.Module.eval() at
 *   avt_bn_eval_bwd_mask,        test.py:85): the backward of the per-channel affine map, with the mask from y / the
 *   avt_stem_*_eval_bwd          pre-activation, from the avt_bn_apply_mask bits, and through the stem's max-pool
 *   (avt_set_*: A/B knobs between measured kernel variants, in avt_tuning.h -- not part of this boundary)
 *   avt_audio_pool_norm_fwd/bwd  nn.AdaptiveMaxPool2d((1,1)) + F.normalize(dim=1) (model.py:96, 120-122)
 *   avt_hardway_fwd/bwd          AVENet.forward head: normalize, A/A0 einsums, sigmoid trimap,
 *                                sim1/sim/sim2, logits/0.07, weighted_A (model.py:114-154);
 *                                HardWayAttention.forward (model.py:46-60)
 *   avt_hardway_ce               nn.CrossEntropyLoss()(logits, zeros) (train_hardway_1frame.py:113, 130-131)
 *   avt_adam_step                torch.optim.Adam(lr, weight_decay) step (train_hardway_1frame.py:116, 134)
 *   avt_sgd_step_dev             torch.optim.SGD(lr, momentum, dampening, weight_decay, nesterov) step: the optimizer
 *                                of the R3D fine-tuning recipe whose weights train_3D.py:89 loads
 *   avt_cls_pool_fwd/bwd,        the R3D-18's own head, ResNet.forward's avgpool -> view -> fc
 *   avt_cls_fc_fwd/bwd,          (models/resnet3D.py:208-212), with nn.CrossEntropyLoss on class labels and their
 *   avt_softmax_ce               backward: the fused fine-tuning step of a stand-alone trunk (train.R3DTrainStep)
 *   avt_conv3d_fwd               nn.Conv3d fwd of the R3D-18 video trunk (models/resnet3D.py:14-28 conv3x3x3 /
 *                                conv1x1x1, called from BasicBlock.forward 45-61; FullModel.vidnet, model.py:20)
 *   avt_video_stem_im2col,       the R3D stem Conv3d(3,64,(7,7,7),s(1,2,2),p3) (models/resnet3D.py:122-127) as a
 *   avt_pack_conv3d_weight       32-channel Conv2d over the frames (temporal taps folded into channels);
 *   (+ _weights_batched)         the other Conv3d weights' bf16 operands in one launch
 *   avt_maxpool3d_fwd            the R3D stem's nn.MaxPool3d(3, 2, 1) when no_max_pool=False (resnet3D.py:129, 200-201)
 *   avt_bn_finalize_rep          BatchNorm2d over the t-fold repeated spectrogram batch (train_3D.py:128-130)
 *                                computed once per distinct clip
 *   avt_twoview_loss             the 16-frame two-view loss of train_hardway.py:134-142: lw*CE x2, (100-lw)*
 *                                nn.MSELoss(weighted, weighted2), PropagationLoss x2 (losses.py:16-23)
 *   avt_propagation_loss         PropagationLoss.forward (losses.py:22-23) + its gradient
 *   avt_npratio_loss             NPRatio.forward (losses.py:13-14) + its gradient (train_3D.py:113, 135)
 *   avt_flip_l1_loss             FlipLoss.forward (losses.py:34-36) + its gradients
 *   avt_ncthw_to_nhwc_bf16       einops 'b c t h w -> (b t) c h w' of the frames (train_hardway.py:130-131)
 *   avt_localize_ciou,           the test loops' heatmap -> cIoU protocol (train_hardway_1frame.py:195-206,
 *   avt_pair_ciou                utils.Evaluator.cal_CIOU utils.py:209-214, utils.mTC 311-318)
 *   avt_heatmap_upsample         the continuous map of that protocol: cv2.resize + normalize_img (test.py:102-111)
 *   avt_render_overlay           save_image / save_labels: frame + colour-mapped maps -> uint8 HWC (train_3D.py:73-81,
 *                                flow.py:71-84)
 *   avt_spectrogram              the dataset's scipy.signal.spectrogram + log + Normalize(0, 12)
 *   avt_frames_transform         the dataset's frame transform: PIL BICUBIC Resize + crop + flip + ToTensor +
 *                                Normalize (datasets/dataloader.py:47-62)
 *   avt_clip_transform           the two-view dataset's clip transform: clip-consistent Resize / crop / flip, and the
 *                                crop + ColorJitter + Resize + flip of the second view (datasets/dataloader.py:155-181)
 *                                (datasets/dataloader.py:86-96, 252-274)
 */
#ifndef AVT_H_
#define AVT_H_

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define AVT_OK 0
#define AVT_EINVAL -1
#define AVT_EHIP -2

const char* avt_last_error(void);
int avt_abi_version(void);
/* bit mask of how this library was built: AVT_BUILD_DIAG = the timing-diagnostics build (-DAVT_DIAG:
 * environment knobs that drop launches or loads and give WRONG results); bench.py refuses such a build */
#define AVT_BUILD_DIAG 1
int avt_build_flags(void);

/* ---- measured peaks (bench.py's roofline denominators, re-measured in the same run) ---- */
/* back-to-back bf16 MFMA on pseudo-random register operands, one wave per SIMD (256-thread blocks):
 * shape 0 = v_mfma_f32_32x32x16_bf16 (4 accumulators), 1 = v_mfma_f32_16x16x32_bf16 (8); sink:
 * float[blocks*256] (one value per lane, keeps the loop live).  avt_peak_mfma_flops: the FLOPs of one
 * such launch (-1 on bad arguments). */
int avt_peak_mfma(float* sink, int shape, int blocks, int iters, unsigned seed, void* stream);
long long avt_peak_mfma_flops(int shape, int blocks, int iters);
/* dst = src, 16-byte vector loads/stores in a grid-stride loop of `blocks` 256-thread blocks (bytes % 16 == 0) */
int avt_copy16(void* dst, const void* src, size_t bytes, int blocks, void* stream);

/* ---- convolution (implicit GEMM on bf16 MFMA, fp32 accumulate) ---- */
/* BatchNorm statistics (deterministic).  A BN's fp64 accumulator holds a small header and one slot of
 * partial sums per row tile (or persistent block / reduce block) of the launch that accumulates it, each
 * slot element written by exactly one block with plain stores (the column tiles of a row tile write
 * disjoint channel ranges of its slot) -- no atomics, nothing to zero between uses, any
 * contents on entry.  The finalize sums the slots in slot order, so identical inputs give bitwise identical
 * statistics, gradients and updates on every run (model.py:112-154's CPU path is deterministic too).
 * Forward: avt_bn_acc_doubles(rows, C) doubles; backward: avt_bn_bwd_workspace(rows, C) bytes.
 *
 * y[N,P,Q,K] = conv(x[N,H,W,Cp], wpack[K][Kg]); if bn_acc != NULL the fp32 results' batch-norm
 * statistics are stored into bn_acc (avt_bn_acc_doubles(N*P*Q, K) doubles), for avt_bn_finalize.
 * Cp is 1 or 4 (stems, Kg = R*S*Cp rounded up to 32) or a multiple of 32 (Kg = R*S*Cp, at most 49 taps); K % 64 == 0;
 * R, S and pad are independent (any pad >= 0 that leaves an output); stride 1 or 2.  Anything else -- an empty input or
 * output, a negative pad, tensors of 2 GiB or more -- is refused before any launch (DESIGN 6r has the whole table). */
size_t avt_bn_acc_doubles(long long rows, int C);
int avt_conv2d_fwd(const void* x, const void* wpack, void* y, double* bn_acc, int N, int H, int W, int Cp, int K,
                   int R, int S, int stride, int pad, int Kg, void* stream);
/* Inference forward with BatchNorm folded into the conv: y = [relu](conv(x, wpack) + bias[k] (+ residual)).
 * Replaces, in eval mode, the conv -> bn (-> + identity) (-> relu) groups of BasicBlock.forward
 * (models/base_models.py:53-69: conv1/bn1/relu at 56-58, conv2/bn2 at 60-61, downsample at 63-64, += and relu at
 * 66-67) with one launch each: wpack is the image avt_fold_conv_bn_batched writes (w * gamma/sqrt(var + eps)),
 * bias its beta - mean * scale, so no pre-BN tensor is stored and no avt_bn_apply pass runs.
 * The arguments are avt_conv2d_fwd's (no statistics accumulator) plus bias (fp32 [K], required), residual (bf16
 * [N,P,Q,K] or NULL; must not alias y) and relu (0 / 1).  The bias is added to the fp32 accumulators before the
 * first bf16 rounding in every kernel form; the layer-1 kernel also adds the residual there, the other forms add it
 * in the store epilogue to the rounded value.  Runs the kernel form avt_conv2d_fwd's planner picks for
 * the shape; no split-K.  Refuses a NULL bias, K % 64 != 0, C % 32 != 0 (the 7x7 stems keep avt_conv2d_fwd and
 * avt_stem_bn_relu_maxpool_fwd), more than 9 taps, Kg != R*S*C, strides other than 1 and 2, tensors of 2 GiB or more. */
int avt_conv2d_fwd_bias(const void* x, const void* wpack, void* y, int N, int H, int W, int Cp, int K, int R, int S,
                        int stride, int pad, int Kg, const float* bias, const void* residual, int relu, void* stream);
/* dx[N,H,W,C] = dgrad(dy[N,P,Q,K], wt[C][R*S*K]) (+ add[N,H,W,C] if add != NULL; add may alias dx).  C % 64 == 0,
 * K % 32 == 0, R and S independent, stride 1 or 2; at most 9 taps per launch -- R*S <= 9 at stride 1, and at stride 2
 * ceil(R/2)*ceil(S/2) <= 9 with R*S <= 32 (a 5x5 / stride 2 is taken, a 5x5 / stride 1 refused: the 2-D kernels'
 * argument block holds nine taps); 0 <= pad < min(R, S) (the bound avt_conv3d_dgrad has); a non-empty dy.
 * So for _mask, _ws and _bn below. */
int avt_conv2d_dgrad(const void* dy, const void* wt, void* dx, const void* add, int N, int H, int W, int C, int K,
                     int R, int S, int stride, int pad, void* stream);
/* dx = dgrad(dy, wt) + add * mask: an identity BasicBlock's input gradient (base_models.py:64-67), the
 * residual branch entering as g * [out > 0] with the bits of avt_bn_apply_mask ([N*H*W][C/8] u8) --
 * the masked copy of g is never stored.  add must not alias dx. */
int avt_conv2d_dgrad_mask(const void* dy, const void* wt, void* dx, const void* add, const void* add_mask, int N,
                          int H, int W, int C, int K, int R, int S, int stride, int pad, void* stream);
/* Split-K form of the 3x3/s1 fwd / dgrad at short grids (a few clips per GPU: layer3/4 of BASELINE
 * configs[2]'s 32-clip shard), same results to fp32 summation order.  avt_conv2d_splitk_plan gives
 * the workspace of one call: part = float[*part_floats] (any contents), cnt = int[*counters] zeroed
 * once (the kernel leaves it zero; one per concurrently running call); both 0 = no split for this
 * shape (the _ws calls then behave as avt_conv2d_fwd / avt_conv2d_dgrad[_mask]).  dgrad: 0 fwd, 1 dgrad.
 * avt_set_halo_splitk(s, blocks): s > 0 forces the split count (largest chunk-count divisor <= s),
 * 0 plans it as the smallest divisor whose grid reaches `blocks` (0: two per CU). */
int avt_conv2d_splitk_plan(int N, int H, int W, int C, int K, int R, int S, int stride, int pad, int dgrad,
                           long long* part_floats, int* counters);
/* part_floats / counters: the sizes of part and cnt as allocated; the plan is re-made at every call from the
 * current knobs, and a call whose plan needs more than the workspace holds runs without split-K. */
int avt_conv2d_fwd_ws(const void* x, const void* wpack, void* y, double* bn_acc, int N, int H, int W, int Cp, int K,
                      int R, int S, int stride, int pad, int Kg, float* part, long long part_floats, int* cnt,
                      int counters, void* stream);
int avt_conv2d_dgrad_ws(const void* dy, const void* wt, void* dx, const void* add, const void* add_mask, int N,
                        int H, int W, int C, int K, int R, int S, int stride, int pad, float* part,
                        long long part_floats, int* cnt, int counters, void* stream);
/* avt_conv2d_dgrad with the backward of the BatchNorm (+ReLU) that produced dx's positions fused into
 * its store epilogue (BasicBlock.forward, base_models.py:46-49, 58-67): the result g (after `add`) is
 * masked, g' = g * [y > 0] (y given: the block output) or g * [fma(xc, scale, shift) > 0] (y NULL:
 * BasicBlock.bn1's ReLU), dx = g' is stored, and sum g', sum g' * (xc - mean) * invstd are stored into
 * acc (an avt_bn_bwd_workspace(N*H*W, C) workspace); xc2/stats2/acc2 (optional) a second BN fed by the
 * same g' (a first block's downsample.1).  skip_class00: for a stride-2 dgrad, the (even, even) pixels are
 * stored plain (a later in-place downsample dgrad finishes them).  append_slots: this call's partial sums
 * go after those of the call before it on acc (that skip_class00 call: the downsample dgrad finishing the
 * same BN's reduction); 0: this call's sums replace whatever acc held. */
typedef struct {
  const void* xc;      /* [N,H,W,C] bf16 pre-BN activations */
  const void* y;       /* [N,H,W,C] bf16 ReLU output, or NULL */
  const float* stats;  /* [4][C] fp32: scale, shift, mean, invstd (avt_bn_finalize outputs) */
  double* acc;
  const void* xc2;
  const float* stats2;
  double* acc2;
  int skip_class00;
  int append_slots;
} avt_dgrad_bn_epi;
int avt_conv2d_dgrad_bn(const void* dy, const void* wt, void* dx, const void* add, int N, int H, int W, int C, int K,
                        int R, int S, int stride, int pad, const avt_dgrad_bn_epi* epi, void* stream);
/* dw[K][R][S][Creal] += wgrad(x[N,H,W,Cp], dy[N,P,Q,K]).  Split-K partials go through an fp32 slab
 * in `workspace` (>= avt_conv2d_wgrad_workspace(...) bytes; deterministic) or, if it is NULL/too
 * small or for the stems, are added with fp32 atomics.  K % 64 == 0; Cp % 8 == 0 with Creal == Cp (or the stems' Cp
 * 4 / 1 with Creal <= Cp); R, S, pad independent, stride 1 or 2; an empty input, output or tap set is refused -- by
 * every wgrad entry point below and by the two size queries' planner alike. */
size_t avt_conv2d_wgrad_workspace(int N, int H, int W, int Cp, int Creal, int K, int R, int S, int stride, int pad);
int avt_conv2d_wgrad(const void* x, const void* dy, float* dw, int N, int H, int W, int Cp, int Creal, int K, int R,
                     int S, int stride, int pad, void* workspace, size_t ws_bytes, void* stream);
/* Deferred split-K reduce: avt_conv2d_wgrad_defer runs the wgrad kernel and, where avt_conv2d_wgrad would launch its
 * separate slab reduce (one wave per slab position), leaves it: *desc describes the slab (desc->splits > 0; keep the
 * workspace alive) and dw is incomplete until avt_wgrad_reduce_batch(descs, n) sums any number of such slabs in one
 * launch (blockIdx.y = the slab), in the same split order (the same bits).  desc->splits == 0: dw is complete. */
typedef struct {
  const float* slab;
  float* dw;
  int splits, tiles, nnt, Mg, ldw;
  int wm, wn, tm, tn;  /* the wgrad tile's wave grid and 32x32 blocks per wave (register order of the partials) */
} avt_slab_reduce_desc;
int avt_conv2d_wgrad_defer(const void* x, const void* dy, float* dw, int N, int H, int W, int Cp, int Creal, int K,
                           int R, int S, int stride, int pad, void* workspace, size_t ws_bytes, avt_slab_reduce_desc* desc,
                           void* stream);
int avt_wgrad_reduce_batch(const avt_slab_reduce_desc* descs, int n, void* stream);
/* The same with the slab summed inside the wgrad kernel: the last block of each output tile to take its ticket adds
 * the tile's split partials into dw in split order (the separate reduce's order: the same bits), so the reduce launch
 * goes.  `tickets`: >= avt_conv2d_wgrad_tickets(...) ints, zero on entry, left zero (keep them for the next call);
 * NULL or a count of 0: avt_conv2d_wgrad.  avt_conv2d_wgrad_tickets() is 0 unless avt_set_wgrad_fused(1) -- the fused
 * form measured slower than the separate reduce (an A/B knob, include/avt_tuning.h). */
int avt_conv2d_wgrad_tickets(int N, int H, int W, int Cp, int Creal, int K, int R, int S, int stride, int pad);
int avt_conv2d_wgrad_tk(const void* x, const void* dy, float* dw, int N, int H, int W, int Cp, int Creal, int K, int R,
                        int S, int stride, int pad, void* workspace, size_t ws_bytes, int* tickets, int n_tickets,
                        void* stream);
/* Per-pixel gather table of the tap-gather wgrad (3x3 / 1x1 convs with Cp % 8 == 0; the stems have their own kernel).
 * One 8-byte entry per output pixel (n, oh, ow), pixel-major, padded with always-invalid (0, 0) entries to a multiple
 * of 32 pixels: a u32 byte offset of input pixel (n, oh*stride - pad, ow*stride - pad) in x[N][H][W][Cp] bf16 (modulo
 * 2^32: it may lie before the tensor; only taps inside the image are dereferenced) and a u32 mask whose bit r*S + s is
 * set where tap (r, s) of that pixel lands inside the image.  It depends on the geometry only -- not on x's address, not
 * on the weights -- so it is built once per geometry and shared by every conv of that geometry:
 *   avt_wgrad_pixtab_bytes()    the table's size, 0 where the form does not apply (more than 32 taps)
 *   avt_wgrad_pixtab_build()    fills `tab` (a launch on `stream`: never inside a graph capture, never per step)
 *   avt_wgrad_pixtab_register() tells the wgrad entry points above to read `tab` for this geometry on the current
 *                               device; the caller keeps it alive and unchanged until it registers NULL (or another
 *                               table) for the geometry.
 * With a registered table the wgrad kernel loads its gather offsets instead of recomputing them per k-tile: the same
 * products in the same order, bitwise-equal results (avt_set_wgrad_pixtab(0), include/avt_tuning.h, ignores the tables). */
size_t avt_wgrad_pixtab_bytes(int N, int H, int W, int R, int S, int stride, int pad);
int avt_wgrad_pixtab_build(void* tab, int N, int H, int W, int Cp, int R, int S, int stride, int pad, void* stream);
int avt_wgrad_pixtab_register(const void* tab, int N, int H, int W, int Cp, int R, int S, int stride, int pad);

/* Input gradient of the 7x7 / stride 2 / pad 3 stem conv (base_models.py:135-138, the reference's autograd through
 * conv1 / conv1_a when the trunk input requires grad): gx[N][Cin][H][W] fp32 (NCHW, the input's layout) =
 * conv2d_input(gy[N,P,Q,64] bf16, w fp32 OHWI [64][7][7][Cin]); Cin <= 4; fp32 sums over (r, s, k) in a fixed order. */
int avt_conv_stem_dgrad(const void* gy, const float* w, float* gx, int N, int H, int W, int Cin, void* stream);

/* Conv3d, temporal stride 1: y[N,T',P,Q,K] = conv3d(x[N,T,H,W,Cp], wpack[K][(kt,r,s,c)]),
 * T' = T + 2*pad_t - KT + 1, spatial stride 1 or 2; Cp % 32 == 0; K % 64 == 0; KT*R*S <= 49 (KT, R, S, pad_t, pad independent);
 * bn_acc as conv2d_fwd */
int avt_conv3d_fwd(const void* x, const void* wpack, void* y, double* bn_acc, int N, int T, int H, int W, int Cp,
                   int K, int KT, int R, int S, int stride, int pad_t, int pad, void* stream);
/* Inference Conv3d with BatchNorm3d folded in: y = [relu](conv3d(x, wpack) + bias[k] (+ residual)).  Replaces, in eval
 * mode, the conv -> bn (-> + residual) (-> relu) groups of the R3D-18 (models/resnet3D.py: BasicBlock.forward 45-61,
 * the stem conv1/bn1/relu of ResNet.forward 198-200) with one launch each: wpack is the image
 * avt_fold_conv3d_bn_batched writes, bias its beta - mean * scale; no pre-BN tensor is stored, no avt_bn_apply runs.
 * The arguments are avt_conv3d_fwd's without the statistics accumulator, plus bias (fp32 [K], required), residual
 * (bf16 [N,T',P,Q,K] or NULL; must not alias y) and relu (0 / 1).  The fp32 bias joins the fp32 accumulators before
 * the first bf16 rounding; residual and ReLU are applied in the store to the rounded value.  Runs the
 * kernel form avt_conv3d_fwd's planner picks for the shape (the halo kernel's three-patch form, else the tap-gather
 * kernel's Conv3d form; a T = KT = 1 conv of at most 9 taps goes where avt_conv2d_fwd_bias sends it).  The folded
 * 7x7x7 video stem is the KT = 1, 7x7 / stride 2 conv over the N*T frames of avt_video_stem_im2col's 32-channel
 * input (49 taps).  Refuses a NULL bias, an aliasing residual, K % 64 != 0, Cp % 32 != 0, more than 49 taps, strides
 * other than 1 and 2, tensors of 2 GiB or more, and a build without the LDS-DMA conv variant. */
int avt_conv3d_fwd_bias(const void* x, const void* wpack, void* y, int N, int T, int H, int W, int Cp, int K, int KT,
                        int R, int S, int stride, int pad_t, int pad, const float* bias, const void* residual,
                        int relu, void* stream);
/* Fold frozen BatchNorm3d's into the Conv3d's in front of them, one launch for the whole R3D trunk: descs = device
 * array of n records {const float* w; void* out; const float *gamma, *beta, *running_mean, *running_var; float* bias;
 * int K, C, KT, R, S, stem; float eps; int pad;} (avt_fold3d_desc_bytes() each), w fp32 OIDHW.  With s[k] = gamma[k] *
 * rsqrt(running_var[k] + eps) (the sum in fp32, its rsqrt as (float)(1 / sqrt((double)sum)): reproducible on any IEEE
 * host): out[k][t*C + c] = bf16(w[k][c][t] * s[k]) (t = (kt, r, s); the layout of
 * avt_pack_conv3d_weights_batched; fp32 product, one rounding), or for a stem record (C <= 4, KT <= 8) the fold-1
 * layout [K][(r,s)][kt*4+c] of avt_pack_conv3d_weight, zero padded; bias[k] = beta[k] - running_mean[k] * s[k].
 * max_k = the largest K, max_row = the largest C*KT*R*S (<= 15360).  No host sync; deterministic. */
size_t avt_fold3d_desc_bytes(void);
int avt_fold_conv3d_bn_batched(const void* descs, int n, int max_k, int max_row, void* stream);
/* R3D stem input: x fp32 NCDHW [N][C<=4][T][H][W] -> bf16 [N][T][H][W][32], channel kt*4+c = x[c][t+kt-pad_t]
 * (zero outside the clip / for c >= C / channels >= 4*KT) */
int avt_video_stem_im2col(const float* x, void* out, int N, int C, int T, int H, int W, int KT, int pad_t,
                          void* stream);
/* w fp32 OIDHW [K][C][KT][R][S] -> bf16 [K][(kt,r,s,c)] (fold 0) or the stem layout
 * [K][(r,s)][kt*4+c] with 32 channels per (r,s) (fold 1) */
int avt_pack_conv3d_weight(const float* w, void* out, int K, int C, int KT, int R, int S, int fold, void* stream);
/* every non-stem Conv3d weight in one launch: descs = device array of n records {const float* w; void* out; int K,
 * C, T, pad} (avt_pack3d_desc_bytes() bytes each), out[k][t*C + c] = bf16(w[k][c][t]) (T = KT*R*S, the fold-0 layout
 * of avt_pack_conv3d_weight); max_k = the largest K, max_row = the largest C*T (<= 15360) */
size_t avt_pack3d_desc_bytes(void);
int avt_pack_conv3d_weights_batched(const void* descs, int n, int max_k, int max_row, void* stream);
/* nn.MaxPool3d(kernel_size=3, stride=2, padding=1) over bf16 NDHWC [N][T][H][W][C], C % 8 == 0 ->
 * [N][(T-1)/2+1][(H-1)/2+1][(W-1)/2+1][C] (the winning input's bits; NaN propagates) */
int avt_maxpool3d_fwd(const void* x, void* y, int N, int T, int H, int W, int C, void* stream);

/* ---- Conv3d backward: the trainable R3D-18 trunk (autograd through models/resnet3D.py:14-20 conv3x3x3 / conv1x1x1 in
 * BasicBlock.forward 45-61, the stem's MaxPool3d :129 and ResNet.forward 197-213).  Conventions of the forward
 * entries: NDHWC bf16 activations, temporal stride 1, spatial stride 1 or 2, Cp % 32 == 0, K % 64 == 0, fp32 sums. */
/* w fp32 OIDHW [K][C][KT][R][S] -> bf16 out[c][(KT-1-kt, R-1-r, S-1-s, k)]: avt_pack_conv3d_weight's fold-0 layout
 * with K and C swapped and the taps reversed -- the weight operand of avt_conv3d_dgrad (the weight transposition of
 * autograd's conv3d input gradient, resnet3D.py:14-20).  K % 64 == 0, at most 64 taps. */
int avt_pack_conv3d_weight_dgrad(const float* w, void* out, int K, int C, int KT, int R, int S, void* stream);
/* ... for a device table of n avt_pack3d_desc_bytes() records in one launch (record.out = that conv's dgrad operand
 * [C][T*K]; max_blocks = the largest C*K/64): the trunk's weights change every step once it trains */
int avt_pack_conv3d_weights_dgrad_batched(const void* descs, int n, int max_blocks, void* stream);
/* dx[N,T,H,W,C] = conv3d_input(dy[N,T',P,Q,K], wt) (+ add[N,T,H,W,C] if add != NULL; add may alias dx): the input
 * gradient of conv3x3x3 (resnet3D.py:14-20; BasicBlock.forward 45-61, `out += residual` :58 entering as `add`).
 * Stride 1 runs avt_conv3d_fwd's kernels (its three-patch halo form included) on dy with pad' = k-1-pad; stride 2
 * walks, per (h%2, w%2) parity class of dx, only the class's spatial taps times the KT temporal taps.  Frames outside
 * a clip contribute zero.  C % 64 == 0, K % 32 == 0, at most 49 taps, pad_t < KT, pad < min(R, S); at stride 1 square
 * spatial taps only (R == S: one pad' serves both axes of the forward form). */
int avt_conv3d_dgrad(const void* dy, const void* wt, void* dx, const void* add, int N, int T, int H, int W, int C, int K,
                     int KT, int R, int S, int stride, int pad_t, int pad, void* stream);
/* dw[K][Cp][KT][R][S] (fp32 OIDHW, the Parameter's layout) += conv3d_weight(x[N,T,H,W,Cp], dy[N,T,P,Q,K]): the weight
 * gradient of conv3x3x3 (resnet3D.py:14-20).  Temporal 'same' padding (T' == T).  Every split-K partial goes through
 * the fp32 slab in `workspace` (>= avt_conv3d_wgrad_workspace(...) bytes, 16-byte aligned, any contents) and is summed
 * in split order: bitwise reproducible; there is no atomic path -- a NULL or short workspace is AVT_EINVAL. */
size_t avt_conv3d_wgrad_workspace(int N, int T, int H, int W, int Cp, int K, int KT, int R, int S, int stride, int pad_t,
                                  int pad);
int avt_conv3d_wgrad(const void* x, const void* dy, float* dw, int N, int T, int H, int W, int Cp, int K, int KT, int R,
                     int S, int stride, int pad_t, int pad, void* workspace, size_t ws_bytes, void* stream);
/* gx[N,T,H,W,C] = backward of avt_maxpool3d_fwd (nn.MaxPool3d(3, 2, 1), resnet3D.py:129, 200-201) under
 * gy[N,To,Ho,Wo,C]: each input voxel sums the gy of the at most 8 windows it wins (no atomics); a window's winner is
 * its first maximum in (t, h, w) scan order, recomputed from x (torch's CPU max_pool3d choice).  y is not read. */
int avt_maxpool3d_bwd(const void* gy, const void* x, const void* y, void* gx, int N, int T, int H, int W, int C,
                      void* stream);
/* R3D stem Conv3d(3,64,(7,7,7),s(1,2,2),p3) weight gradient (resnet3D.py:122-127): dwf fp32 [K][R][S][32] is
 * avt_conv2d_wgrad's result over the folded input of avt_video_stem_im2col (Cp = Creal = 32, with its workspace:
 * deterministic); dw[k][c][kt][r][s] (fp32 OIDHW [K][C][KT][R][S]) += dwf[k][r][s][kt*4 + c] */
int avt_stem3d_wgrad_unfold(const float* dwf, float* dw, int K, int C, int KT, int R, int S, void* stream);
/* R3D stem Conv3d(3,64,(7,7,7),s(1,2,2),p3) input gradient (resnet3D.py:122-127 under autograd, when the video requires
 * grad): gx[N][3][T][H][W] fp32 (NCDHW, the video's layout) = conv3d_input(gy[N,T,P,Q,64] bf16, w), P = (H-1)/2+1,
 * Q = (W-1)/2+1; frames outside the clip and rows/columns outside the frame contribute zero.  Two forms behind
 * avt_set_video_stem_dgrad (avt_tuning.h): 0 = direct, fp32 weights w (OIDHW [64][3][7][7][7]), fp32 sums over
 * (kt, r, s, k) in a fixed order; 1 = MFMA, the transpose of the forward's folded 2-D conv per (h%2, w%2) parity class
 * with the temporal fold-back fused (no intermediate), weights rounded to bf16 in the operand `wpack`
 * (avt_video_stem_dgrad_pack_bytes() bytes, 16-byte aligned, written by avt_pack_video_stem_dgrad -- once per step),
 * fp32 accumulation.  Only the selected form's weight argument is read; no atomics, bitwise reproducible. */
size_t avt_video_stem_dgrad_pack_bytes(void);
int avt_pack_video_stem_dgrad(const float* w, void* out, void* stream);
int avt_video_stem_dgrad(const void* gy, const float* w, const void* wpack, float* gx, int N, int T, int H, int W,
                         void* stream);

/* tube-step audio de-duplication: out[b*rep+k][:] = in[b][:]  /  out[b][:] = sum_k in[b*rep+k][:] */
int avt_repeat_rows_f32(const float* in, float* out, int B, int rep, int C, void* stream);
int avt_sum_rep_rows_f32(const float* in, float* out, int B, int rep, int C, void* stream);

/* ---- batch norm (train mode) ---- */
/* merge bn_acc (see avt_conv2d_fwd) over `rows` rows -> scale, shift, mean, invstd (fp32 [C]);
 * running stats updated if non-NULL (momentum, unbiased var); bn_acc is read, not modified */
int avt_bn_finalize(double* acc, long long rows, int C, const float* gamma, const float* beta, float* running_mean,
                    float* running_var, float momentum, float eps, float* scale, float* shift, float* save_mean,
                    float* save_invstd, void* stream);
/* avt_bn_finalize for a logical batch in which each accumulated row occurs `rep` times: the running
 * variance uses the unbiased factor of rows*rep rows (mean/variance are those of the distinct rows) */
int avt_bn_finalize_rep(double* acc, long long rows, long long rep, int C, const float* gamma, const float* beta,
                        float* running_mean, float* running_var, float momentum, float eps, float* scale,
                        float* shift, float* save_mean, float* save_invstd, void* stream);
/* out = [relu](x*scale+shift + [residual*rscale+rshift | residual]) over rows x C (NHWC rows) */
int avt_bn_apply(const void* x, const float* scale, const float* shift, const void* residual, const float* rscale,
                 const float* rshift, void* out, long long rows, int C, int relu, void* stream);
/* avt_bn_apply with relu, also writing the ReLU mask of out as bits: mask [rows][C/8] u8, bit e of byte
 * j = out[.][8j+e] > 0 (the stored bf16 value) -- what the backward's relu mask reads instead of out */
int avt_bn_apply_mask(const void* x, const float* scale, const float* shift, const void* residual, const float* rscale,
                      const float* rshift, void* out, void* mask, long long rows, int C, void* stream);
/* bytes of the BN-backward workspace for up to `rows` rows (any contents on entry) */
size_t avt_bn_bwd_workspace(long long rows, int C);
/* g' = g*[y>0] (y may be NULL: no mask); dgamma += sum g'*xhat; dbeta += sum g';
 * gc = gamma*invstd*(g' - mean(g') - xhat*mean(g'*xhat)); gmask_out (optional) = g' */
int avt_bn_bwd(const void* g, const void* y, const void* xc, const float* mean, const float* invstd,
               const float* gamma, float* dgamma, float* dbeta, void* gc, void* gmask_out, void* workspace,
               long long rows, int C, void* stream);
/* one BatchNorm fed by g' (see avt_bn_bwd_mask) */
typedef struct {
  const void* xc;         /* [rows][C] bf16 pre-BN activations */
  const float* mean;      /* [C] batch mean / invstd (avt_bn_finalize save_mean / save_invstd) */
  const float* invstd;
  const float* gamma;
  float* dgamma;          /* [C] accumulated (+=), may be NULL */
  float* dbeta;
  void* gc;               /* [rows][C] bf16 output: gradient of xc */
  void* workspace;        /* avt_bn_bwd_workspace(rows, C) bytes (any contents on entry) */
} avt_bn_bwd_target;
/* BasicBlock output backward (base_models.py:64-67): g' = g * mask (bits of avt_bn_apply_mask), then the
 * BN backward of t1 and -- if t2 != NULL -- of t2 (a first block's bn2 and downsample.1, which share g'),
 * reading g and the mask once for both */
int avt_bn_bwd_mask(const void* g, const void* mask, const avt_bn_bwd_target* t1, const avt_bn_bwd_target* t2,
                    long long rows, int C, void* stream);
/* Eval-mode (running-statistics) BatchNorm backward, one pass: g' = g * mask; per target (t2 optional, sharing g': a
 * first block's bn2 + downsample.1) gc = gamma*invstd*g', dbeta += sum g', dgamma += sum g'*(xc - mean)*invstd with
 * mean = running_mean, invstd = rsqrt(running_var + eps) -- no mean-subtraction terms.  Mask: y > 0 if y != NULL, else
 * fma(t1->xc, mscale, mshift) > 0 if mscale != NULL (as avt_bn_relu_bwd), else none; gmask_out (optional) = g'.  The
 * sums go through the target's fixed-order slot workspace (avt_bn_bwd_workspace; bitwise reproducible); a target with
 * dgamma == dbeta == NULL needs no workspace and is purely elementwise. */
int avt_bn_eval_bwd(const void* g, const void* y, const float* mscale, const float* mshift, const avt_bn_bwd_target* t1,
                    const avt_bn_bwd_target* t2, void* gmask_out, long long rows, int C, void* stream);
/* avt_bn_eval_bwd with g' = g * mask bits ([rows][C/8] u8 of avt_bn_apply_mask: bit e of byte j is channel 8j+e) -- the
 * backward of a 2-D BasicBlock output under running statistics; t2 (optional) shares g' (bn2 + downsample.1: g and the
 * mask are read once for both).  Rows are dealt and the sums ordered as in avt_bn_eval_bwd: where the bits equal
 * [out > 0] the results are those of avt_bn_eval_bwd(y = out) bit for bit.  A target with dgamma == dbeta == NULL needs
 * no workspace and reduces nothing. */
int avt_bn_eval_bwd_mask(const void* g, const void* mask, const avt_bn_bwd_target* t1, const avt_bn_bwd_target* t2,
                         long long rows, int C, void* stream);
/* avt_bn_bwd for a g' that is already masked and whose reductions a dgrad epilogue already added
 * into the workspace (avt_conv2d_dgrad_bn): finalize + apply only */
int avt_bn_bwd_premasked(const void* gm, const void* xc, const float* mean, const float* invstd, const float* gamma,
                         float* dgamma, float* dbeta, void* gc, void* workspace, long long rows, int C, void* stream);
/* as avt_bn_bwd with g' = g*[fma(xc, scale, shift) > 0] -- the ReLU mask the forward's avt_bn_apply
 * produced from the same (scale, shift), recomputed instead of read */
int avt_bn_relu_bwd(const void* g, const void* xc, const float* scale, const float* shift, const float* mean,
                    const float* invstd, const float* gamma, float* dgamma, float* dbeta, void* gc, void* workspace,
                    long long rows, int C, void* stream);
/* stem: y = maxpool3s2(relu(c*scale + shift)) without storing the full-resolution activation; idx = window
 * argmax (as avt_maxpool3s2_fwd), carg = c at the argmax.  y/idx/carg are [N,P,Q,C] */
int avt_stem_bn_relu_maxpool_fwd(const void* c, const float* scale, const float* shift, void* y, void* idx,
                                 void* carg, int N, int H, int W, int C, void* stream);
/* gc = bn_bwd(relu_bwd(maxpool_bwd(gy))) over the [N,H,W,C] pre-activation c (workspace: avt_bn_bwd_workspace) */
int avt_stem_maxpool_bn_relu_bwd(const void* gy, const void* idx, const void* carg, const void* c, const float* scale,
                                 const float* shift, const float* mean, const float* invstd, const float* gamma,
                                 float* dgamma, float* dbeta, void* gc, void* workspace, int N, int H, int W, int C,
                                 void* stream);
/* the stem backward under running statistics (mean = running_mean, invstd = rsqrt(running_var + eps)), one pass from
 * the pooled gradient gy [N,P,Q,C] to gc [N,H,W,C]: gc = gamma*invstd * [fma(c, scale, shift) > 0] * (sum of gy over the
 * windows whose idx selects the pixel) -- no mean terms; a pixel no window selects gets +0.  dgamma / dbeta (optional,
 * accumulated): sum g'*(carg - mean)*invstd / sum g' over the pooled rows, through the fixed-order slot workspace
 * (avt_bn_bwd_workspace(N*H*W, C), bitwise reproducible); both NULL: carg, mean and workspace are not read.
 * Shape limits as avt_stem_maxpool_bn_relu_bwd. */
int avt_stem_maxpool_bn_relu_eval_bwd(const void* gy, const void* idx, const void* carg, const void* c,
                                      const float* scale, const float* shift, const float* mean, const float* invstd,
                                      const float* gamma, float* dgamma, float* dbeta, void* gc, void* workspace, int N,
                                      int H, int W, int C, void* stream);

/* ---- pooling ---- */
int avt_maxpool3s2_fwd(const void* x, void* y, void* idx, int N, int H, int W, int C, void* stream);
int avt_maxpool3s2_bwd(const void* gy, const void* idx, void* gx, int N, int H, int W, int C, void* stream);
int avt_audio_pool_norm_fwd(const void* a, float* an, int* amax, float* anorm, int B, int HW, int C, void* stream);
int avt_audio_pool_norm_bwd(const float* gan, const float* an, const int* amax, const float* anorm, void* ga, int B,
                            int HW, int C, void* stream);

/* ---- hard-way head (fp32) ---- */
size_t avt_hardway_save_floats(int B);
int avt_hardway_fwd(const void* v, const float* an, int B, int P, int C, float eps1, float eps2, float tau, int trimap,
                    int use_neg, float* inv, float* vsum, float* A0, float* save, float* logits, float* Aout,
                    float* Pos, float* Neg, float* wA, void* stream);
int avt_hardway_ce(const float* logits, int B, int L, float scale, float* loss, float* dlogits, void* stream);
/* dvh = gv = NULL: no vision gradient (detached video features of the tube head).
 * dwA [B][P] (or NULL): upstream gradient of weighted_A (model.py:148-152; train_hardway.py:138-141
 * back-propagates it), needs the forward's vsum and a dm [B][P] workspace.
 * gan_accumulate = 1: gan += (two views sharing one audio batch) instead of gan = */
int avt_hardway_bwd(const void* v, const float* an, const float* inv, const float* A0, const float* save,
                    const float* dlogits, int B, int P, int C, float eps1, float eps2, float tau, int trimap,
                    int use_neg, const float* dwA, const float* vsum, float* dm, float* dA0, float* dvh, void* gv,
                    float* gan, int gan_accumulate, void* stream);
/* avt_hardway_bwd plus the gradients arriving through the returned maps A, Pos, Neg (model.py:154;
 * gA/gPos/gNeg [B][P] fp32, each may be NULL) */
int avt_hardway_bwd_ex(const void* v, const float* an, const float* inv, const float* A0, const float* save,
                       const float* dlogits, int B, int P, int C, float eps1, float eps2, float tau, int trimap,
                       int use_neg, const float* dwA, const float* vsum, float* dm, const float* gA, const float* gPos,
                       const float* gNeg, float* dA0, float* dvh, void* gv, float* gan, int gan_accumulate,
                       float* ws, void* stream);
/* ws (avt_hardway_bwd_ex / avt_hardway_attention_bwd): avt_hardway_bwd_ws_floats(B, C) floats for the split-K
 * partials of the audio-vector gradient, summed in split order (deterministic); NULL: one split (slow).
 * avt_hardway_bwd runs without it. */
size_t avt_hardway_bwd_ws_floats(int B, int C);
/* Standalone HardWayAttention()(audio_features, video_features) -> (A, logits) (model.py:38-60): fp32
 * features taken as given (the module does not normalise them; FullModel normalises before the call,
 * model.py:31-35), tri-map and Neg on.  v [B][P][C] fp32 = '(b t) (h w) c' of video_features,
 * an [B][C] fp32.  inv/vsum [B][P], A0 [B][P][B], save [B*(2B+4)] are saved for the backward; Pos, Neg,
 * wA [B][P] are scratch. */
int avt_hardway_attention_fwd(const float* v, const float* an, int B, int P, int C, float eps1, float eps2, float tau,
                              float* inv, float* vsum, float* A0, float* save, float* logits, float* Aout, float* Pos,
                              float* Neg, float* wA, void* stream);
/* Its backward: dlogits [B][B+2] and gA [B][P] (or NULL) -> gv [B][P][C] fp32 (d video features,
 * '(b t) (h w) c'), gan [B][C] fp32 (d audio features).  dA0 [B][P][B], dvh [B][P][C] fp32: workspace. */
int avt_hardway_attention_bwd(const float* v, const float* an, const float* inv, const float* A0, const float* save,
                              const float* dlogits, const float* gA, int B, int P, int C, float eps1, float eps2,
                              float tau, float* dA0, float* dvh, float* gv, float* gan, float* ws, void* stream);
/* train_hardway.py:134-142 loss combination of the 16-frame two-view step: given the two CE values
 * (avt_hardway_ce outputs; their dlogits use scale loss_weight/2) and weighted_A of both views
 * ([b*t][P], '(b t)' clip-major), out[5] = {combined, hardway, aug, l2, consistency} and
 * dwA1/dwA2 = d(combined)/d(weighted_A).  losses.py:16-23 PropagationLoss + nn.MSELoss. */
int avt_twoview_loss(const float* ce1, const float* ce2, const float* wA1, const float* wA2, int b, int t, int P,
                     float loss_weight, float* out, float* dwA1, float* dwA2, void* stream);
/* Scratch (floats) of the three losses below for n elements / `rows` rows (NPRatio: b*t): per-block
 * partial sums, summed by one block in a fixed order (deterministic) -- and NPRatio's row sums */
size_t avt_loss_workspace_floats(long long n, long long rows);
/* PropagationLoss (losses.py:16-23) of x [b][t][P]; dx (or NULL) = d(loss)/dx */
int avt_propagation_loss(const float* x, int b, int t, int P, float* loss, float* dx, float* ws, void* stream);
/* NPRatio (losses.py:7-14) of x [b][t][P]: mean |diff_t sum_p x|; dx (or NULL) = d(loss)/dx */
int avt_npratio_loss(const float* x, int b, int t, int P, float* loss, float* dx, float* ws, void* stream);
/* FlipLoss (losses.py:25-36): nn.L1Loss()(y, hflip(x)) over `rows` rows of W; dx, dy (or NULL) gradients */
int avt_flip_l1_loss(const float* x, const float* y, long long rows, int W, float* loss, float* dx, float* dy,
                     float* ws, void* stream);

/* ---- classifier head of the stand-alone R3D-18: AdaptiveAvgPool3d((1,1,1)) + fc + CrossEntropyLoss ----
 * (models/resnet3D.py:208-212 `x = self.avgpool(x); x = x.view(x.size(0), -1); x = self.fc(x)` and the class-label loss
 * of the fine-tuning recipe the trunk's Kinetics weights come from, train_3D.py:89).  fp32 throughout except the layer4
 * map and its gradient (bf16).  Every sum runs in a fixed order, no atomics: identical inputs give identical bits.
 *
 * avt_cls_pool_fwd: v bf16 [b][per][C] (the layer4 map, per = t*h*w, C % 8 == 0, 16-byte aligned) -> feat fp32 [b][C] =
 * (sum_p v[b][p][c]) / per.  DIVIDE BY per: the fp32 sum is divided by (float)per with IEEE fp32 division (correctly
 * rounded); no reciprocal is formed, here or in avt_cls_pool_bwd.  `per` is split into slots of 64 rows, one block per
 * (slot, clip, 512 channels); each slot's partial sums are written to the workspace with plain stores and a second
 * launch adds them in slot order.  workspace: avt_cls_pool_ws_bytes(b, per, C) = b * ceil(per / 64) * C * 4 bytes, any
 * contents; NULL or a shorter one is AVT_EINVAL.  1 <= per < 2^24, b <= 65535. */
size_t avt_cls_pool_ws_bytes(int b, long long per, int C);
int avt_cls_pool_fwd(const void* v, float* feat, int b, long long per, int C, void* workspace, size_t ws_bytes,
                     void* stream);
/* g bf16 [b][per][C] = bf16_rne(gfeat[b][c] / per) at every position p (the same fp32 division), 16-byte stores */
int avt_cls_pool_bwd(const float* gfeat, void* g, int b, long long per, int C, void* stream);
/* nn.Linear: logits[b][n] = bias[n] + sum_c feat[b][c] * W[n][c]; W row-major [n][C] (the Parameter's layout), any
 * n >= 1, C >= 1.  One wave per output: lanes strided over c, then the xor-butterfly wave sum, then + bias. */
int avt_cls_fc_fwd(const float* feat, const float* W, const float* bias, float* logits, int b, int C, int n,
                   void* stream);
/* Its backward, stored (not accumulated): gW[n][C] = sum_b dlogits[b][n] * feat[b][c] and gbias[n] = sum_b
 * dlogits[b][n] (b increasing), gfeat[b][C] = sum_n dlogits[b][n] * W[n][c] (n increasing).  Two launches. */
int avt_cls_fc_bwd(const float* dlogits, const float* feat, const float* W, float* gW, float* gbias, float* gfeat, int b,
                   int C, int n, void* stream);
/* nn.CrossEntropyLoss()(logits, labels) * scale, its gradient and the top-1 count: logits fp32 [b][n], labels int64
 * [b] (device).  A label outside [0, n) marks an ignored row, as torch's ignore_index = -100 does for -100: it adds
 * nothing to the loss, its dlogits row is +0 and it does not count in the denominator; the kernel never traps on a
 * label.  loss[0] = scale * mean over the valid rows of (logsumexp(z) - z[label]); dlogits[b][n] (optional) = scale *
 * (softmax(z) - onehot(label)) / (valid rows); correct[0] (optional, int32) = valid rows whose argmax (the lowest index
 * among equal maxima) is the label.  With NO valid row the loss and every gradient are 0 (torch returns NaN there).
 * One block: a wave per row, rows wider than the wave in strided passes; rows and waves are summed in index order. */
int avt_softmax_ce(const float* logits, const long long* labels, int b, int n, float scale, float* loss, float* dlogits,
                   int* correct, void* stream);

/* ---- localisation metrics (test loops of train_hardway*.py / test.py; utils.py:203-239, 311-318) ---- */
/* A [N][h][w] heatmaps -> cv2 INTER_LINEAR resize to S x S, normalize_img(-.), 1 - ., median
 * binarisation, cIoU(., gt, 0.5): out [N][3] fp64 = (cIoU, intersection, denominator) when gt
 * [N][S][S] is given; pred_out [N][S][S] u8 binary maps (either may be NULL, not both) */
int avt_localize_ciou(const float* A, int N, int h, int w, int S, const float* gt, double* out, void* pred_out,
                      void* stream);
/* out[k] = cIoU(p[k], p[k+1], 0.5) of binary maps p [N][n] u8, k < N-1 (utils.mTC) */
int avt_pair_ciou(const void* p, int N, int n, double* out, void* stream);
/* The continuous map avt_localize_ciou binarises, written out: A [N][h][w] -> out [N][S][S] fp32 by the same cv2
 * INTER_LINEAR arithmetic (half-pixel centres, edges clamped with zero weight, horizontal then vertical pass,
 * separately rounded fp32 products and sums).  normalize 0: the plain resize; 1: normalize_img(resize) over each
 * map's own min and max (utils.py:234-239; a constant map is left as it is); -1: 1 - normalize_img(-resize), the
 * `pred` the test loops threshold at its median (test.py:102-111 shows it).  2 <= S <= 512. */
int avt_heatmap_upsample(const float* A, int N, int h, int w, int S, int normalize, float* out, void* stream);

/* ---- qualitative output (save_image: visualize.py:46-50, train_3D.py:73-81; save_labels: flow.py:80-84) ---- */
/* img [N][3][H][W] fp32 (the network's normalised frames) -> out [N][H][W][3] u8.  Per frame, vmin / vmax over its
 * 3 H W values; n = (x - vmin) / (vmax - vmin) (n = x when they are equal), a = fp32(fp32(n * 255) * wimg).  Per
 * layer k, c_k = lut[u8(map_k * scale_k)][ch] (fp32 product, truncated, clamped to [0, 255]); map_k [N][H][W] fp32
 * or NULL, lut [256][3] u8.  out = u8(trunc(double(a) + (c0 * 0.5 + c1 * 0.5) * w0)) with both layers (save_image;
 * w1 is not used and must be 0), u8(trunc(double(a) + c0 * w0)) with map0 alone (save_labels), u8(trunc(a)) with
 * none: the bytes numpy 2.x gives for the reference's expression.  Sums outside [0, 255] saturate (numpy's cast of
 * them is undefined).  Channel ch of the table goes to channel ch of the frame: with cv2's BGR table on an RGB
 * frame, as in the reference, the jet colours come out mirrored (hot = blue).  map1 without map0, a layer without
 * lut and non-positive sizes are refused. */
int avt_render_overlay(const float* img, int N, int H, int W, const float* map0, float scale0, double w0,
                       const float* map1, float scale1, double w1, float wimg, const unsigned char* lut,
                       unsigned char* out, void* stream);

/* ---- flow-compensated temporal consistency (flow.py:133-157; utils.flow2img, utils.py:64-192) ----
 * Everything downstream of "an optical-flow field exists"; the estimator (FlowNet2) is not part of this library.
 *
 * bilinear_at(m [H][W], ix, iy), the one sampling definition of the three entries below: x0 = floor(ix), y0 =
 * floor(iy); nw = (x0+1-ix)*(y0+1-iy), ne = (ix-x0)*(y0+1-iy), sw = (x0+1-ix)*(iy-y0), se = (ix-x0)*(iy-y0); result
 * nw*m[y0][x0] + ne*m[y0][x0+1] + sw*m[y0+1][x0] + se*m[y0+1][x0+1], the terms added in that order starting from the
 * first neighbour inside [0,W) x [0,H); a neighbour outside contributes nothing (zero padding), none inside gives +0,
 * and so does a NaN or infinite ix or iy.  Every difference, product and sum is one separately rounded fp32
 * operation (no FMA).  A finite position of any magnitude is safe (it is clamped before the int conversion).
 *
 * coords selects what a field entry (f0, f1) of output pixel (x, y) means; channel 0 is horizontal:
 *   0 "grid":   grid_sample coordinates, ix = ((f0 + 1) * W - 1) / 2, iy = ((f1 + 1) * H - 1) / 2 (torch's
 *               un-normalisation for align_corners=False, four fp32 operations each).  The output has the field's
 *               own size [Ho][Wo], which may differ from [H][W].  This is flow.py:152 to the letter: the reference
 *               hands FlowNet2's PIXEL displacements to grid_sample as if they were normalised coordinates, so its
 *               own warp samples far outside the map almost everywhere.
 *   1 "pixels": displacements in pixels of the map, ix = x + f0, iy = y + f1 (one fp32 add each); the output has
 *               the map's size.  This is what the metric flow.py:143 cites means.
 * Every field pointer must be 8-byte aligned (both components of an entry are one load); a pointer that is only
 * 4-byte aligned is refused.  All entries: sizes >= 1 and H*W, Ho*Wo <= 2^30; an unknown coords, a NULL pointer or a
 * bad size is refused with AVT_EINVAL before any launch, the outputs untouched.  No float atomics: the same inputs
 * give the same bytes. */
/* bytes of the scratch avt_flow_consistency (maps = T - 1, pixels = S*S) and avt_flow_color (maps = N, pixels = H*W)
 * take: per-chunk counts / maxima of their first launch.  Any contents; 8-byte aligned. */
size_t avt_flow_workspace_bytes(int maps, long long pixels);
/* grid_sample(src, field, mode='bilinear', padding_mode='zeros', align_corners=False) (flow.py:152) or its pixel-
 * displacement form: out[n][y][x] = bilinear_at(src[n], position of (x, y) from field[n][y][x]).  src [N][H][W] fp32
 * (src_u8 = 0) or u8 (src_u8 = 1: a non-zero byte is 1, as avt_pair_ciou reads its maps); field [N][Ho][Wo][2] fp32;
 * out [N][Ho][Wo] fp32.  coords = 1 needs Ho = H and Wo = W. */
int avt_flow_warp(const void* src, int src_u8, int N, int H, int W, const float* field, int Ho, int Wo, int coords,
                  float* out, void* stream);
/* The flow-compensated avt_pair_ciou: pred [T][S][S] u8 binary maps (avt_localize_ciou's pred_out), field
 * [T-1][S][S][2] fp32; out [T-1][3] fp64 = (cIoU, intersection, denominator) of utils.Evaluator.cal_CIOU(warped,
 * pred[k+1], 0.5) (utils.py:209-214): infer = bilinear_at(pred[k]) >= 0.5, gt = pred[k+1], inter = sum infer*gt, denom
 * = sum gt + sum infer*(gt == 0), cIoU = inter / denom (0 / 0 = NaN, as avt_pair_ciou gives).  The warped map is
 * never stored; the sums are integer counts (exact), converted to fp64 for the divide.  With a zero field in pixel
 * coordinates out[k][0] is avt_pair_ciou's out[k] bit for bit.  2 <= T <= 65536, 1 <= S <= 32768. */
int avt_flow_consistency(const void* pred, int T, int S, const float* field, int coords, double* out, void* workspace,
                         void* stream);
/* The trainable counterpart at heat-map resolution (the FlowLoss flow.py:117 constructs and losses.py never defines):
 * x [b][t][h][w] fp32, field [b][t-1][h][w][2] fp32; with d_s(p) = bilinear_at(x[c][s])(p) - x[c][s+1][p] and
 * k = 1 / (float(b) * float(t-1) * float(h*w)),
 *   *loss = k * sum |d_s(p)|: one partial per (clip, pair) into ws (a thread's p = tid, tid + 256, ... in order, then
 *           the 64 lanes of a wave by xor butterfly 32 .. 1, then the 4 waves in order), the partials summed by one
 *           block the same way;
 *   dx (optional) [b][t][h][w]: dx[c][s][q] = (+0 + k * G) - k * sign(d_{s-1}(q)), where G = sum over output pixels p
 *           increasing, corners nw, ne, sw, se, of sign(d_s(p)) * weight(p, corner) for the corners that are q -- the
 *           first bracket for s < t-1 only, the last term for s > 0 only; sign(0) = 0 (torch's abs backward); each
 *           operation rounded separately.  A gather, not a scatter: one block per (clip, frame) keeps the pair's signs,
 *           weights and cell indices in LDS.
 * The field gets no gradient (flow.py:159 backpropagates the hard-way loss alone; the estimator is frozen,
 * flow.py:107).  ws: b*(t-1) floats.  t >= 2; h*w <= 1024 (the model's maps are 14 x 14 and 16 x 16), above it
 * refused. */
int avt_flow_loss(const float* x, int b, int t, int h, int w, const float* field, int coords, float* loss, float* dx,
                  float* ws, void* stream);
/* utils.flow2img (utils.py:155-192) of N fields: field [N][H][W][2] fp32 -> out [N][H][W][3] u8 (RGB).  The field is
 * not modified (the reference overwrites its argument).  Per field in fp64, each operation rounded separately as
 * numpy evaluates it: a component with |.| > 1e7 marks the pixel unknown and both are zeroed; maxrad = max(-1, max
 * sqrt(u^2 + v^2)); u = u / maxrad + 2^-52, likewise v; then compute_color (utils.py:112-154): a NaN u or v zeroes
 * both and flags the pixel; rad = sqrt(u^2 + v^2), a = atan2(-v, -u) / pi, fk = (a + 1) / 2 * 54 + 1, k0 = floor(fk),
 * k1 = k0 + 1 (56 wraps to 1), f = fk - k0; per channel col = (1 - f) * wheel[k0-1] / 255 + f * wheel[k1-1] / 255,
 * col = 1 - rad * (1 - col) where rad <= 1, else col * 0.75; byte = u8(floor(255 * col * (1 - flag))); unknown pixels
 * 0.  wheel [55][3] u8: the Middlebury colour wheel (utils.py:64-111).  An all-zero field has maxrad = 0, every
 * pixel NaN, and comes out black, as in the reference.  One thing is ours: a NaN input does not take part in the
 * maximum (numpy's max would return NaN, Python's max(-1, nan) then -1, and every other pixel of the field would be
 * drawn negated); here the rest of the field is drawn as if that pixel were zero.  The device's fp64 sqrt and atan2
 * need not round as the host's do: a byte may differ by 1 where 255 * col lies within rounding of an integer.
 * workspace: avt_flow_workspace_bytes(N, H*W).  1 <= N <= 65535. */
int avt_flow_color(const float* field, int N, int H, int W, const unsigned char* wheel, unsigned char* out,
                   void* workspace, void* stream);

/* ---- audio front end (datasets/dataloader.py:86-96): waveform -> normalised log-spectrogram ---- */
/* segments of a length-N waveform at hop = nperseg - noverlap (the reference: 512 - 1) */
int avt_spectrogram_segments(long long n_samples, int hop);
/* x [B][N] fp32 -> out [B][1][257][nseg] = log(PSD + 1e-7) / 12 with scipy.signal.spectrogram's
 * defaults (periodic Tukey(0.25), constant detrend, one-sided density scaling), input clipped to [-1,1] */
int avt_spectrogram(const float* x, int B, long long N, int hop, float fs, float* out, void* stream);

/* ---- frame transform (datasets/dataloader.py:47-62): decoded RGB frames -> normalised tensors ----
 * src: uint8 HWC frames packed at byte offsets; desc: DEVICE int64 [n][8] = {offset, H, W, resized_h,
 * resized_w, crop_top, crop_left, flip}; tmp: device scratch of n*3*Hmax*S bytes; mean/std: HOST
 * float[3]; out: float32 [n][3][S][S].  The resize is bit-identical to Pillow's Image.resize(BICUBIC)
 * (fixed-point separable resampler); S <= 256, downscale factor <= 7.5 (checked by the caller). */
int avt_frames_transform(const void* src, const long long* desc, int n, int S, int Hmax, void* tmp,
                         const float* mean, const float* std, float* out, void* stream);

/* ---- two-view clip transform (SubSampledFlickr, datasets/dataloader.py:155-181, 260-263) ----
 * b clips of t frames each (frame k of clip i is entry i*t + k of src / desc) -> the two tensors of the 16-frame
 * two-view step, float32 NCTHW [b][3][t][S][S]:
 *   frames    = Resize(bicubic) -> crop(S) -> flip -> ToTensor -> Normalize         (desc, as avt_frames_transform;
 *               the caller repeats a clip's draw in each of its frames' rows)
 *   augmented = crop(S2 = avt_clip_crop2(S) = int(0.7 S)) of the 8-bit `frames` image -> colour jitter -> Resize(S,
 *               bicubic) -> flip -> ToTensor -> Normalize                            (view2[i], one per clip)
 * The jitter is an ordered chain of at most four ops, each kind at most once, each acting on the previous op's 8-bit
 * result, in Pillow's arithmetic (ImageEnhance.Brightness / Contrast / Color; hue through convert("HSV") with
 * H' = (H + int(255 h)) mod 256, |h| <= 0.5); the contrast mean is per frame, the factor per clip.  Bit-identical
 * to the same pipeline done with Pillow 12.2.0.  view2 == NULL and augmented == NULL: `frames` alone (test mode).
 * desc and view2 are DEVICE tables; mean / std HOST float[3].  Five launches (two for one view), whatever b and t;
 * no atomics.  The checks of avt_frames_transform's caller apply (crop inside the resized frame, downscale <= 7.5,
 * Hmax >= every H), and 0 <= crop_top, crop_left <= S - S2.  workspace: >= avt_clip_workspace_bytes() bytes,
 * 16-byte aligned, any contents; desc / view2 8-byte aligned.  AVT_EINVAL on a bad size, a short workspace or a
 * misaligned pointer. */
#define AVT_JITTER_BRIGHTNESS 0
#define AVT_JITTER_CONTRAST 1
#define AVT_JITTER_SATURATION 2
#define AVT_JITTER_HUE 3
typedef struct {
  int kind; /* AVT_JITTER_* */
  int reserved;
  double factor; /* brightness / contrast / saturation: >= 0 (1 = unchanged); hue: h in [-0.5, 0.5] */
} avt_jitter_op;
typedef struct {
  int crop_top, crop_left, flip, nops;
  avt_jitter_op ops[4];
} avt_clip_view2; /* 80 bytes */
int avt_clip_crop2(int S);
size_t avt_clip_workspace_bytes(int b, int t, int S, int Hmax, int two_views);
int avt_clip_transform(const void* src, const long long* desc, const avt_clip_view2* view2, int b, int t, int S,
                       int Hmax, void* workspace, size_t ws_bytes, const float* mean, const float* std, float* frames,
                       float* augmented, void* stream);

/* ---- optimizer / layout ---- */
int avt_adam_step(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, long long n, float grad_scale,
                  float lr, float beta1, float beta2, float eps, float weight_decay, int step, void* stream);
/* avt_adam_step with the step count AND the hyper-parameters on the device: hyper = device float[5]
 * {lr, beta1, beta2, eps, weight_decay}, read at every launch (a schedule or a restored checkpoint
 * writes it; a captured graph follows); *step is incremented first and the bias corrections computed
 * there into coef[AVT_ADAM_COEF_FLOATS] (scratch) — graph-capturable */
#define AVT_ADAM_COEF_FLOATS 8
int avt_adam_step_dev(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, long long n,
                      float grad_scale, const float* hyper, int* step, float* coef, void* stream);
/* avt_adam_step_dev in two parts (the same update): prep increments *step and writes coef once per
 * step; apply updates one region of the flat buffers from coef (train.py: each trunk's region at the
 * end of that trunk's backward branch) */
int avt_adam_prep_dev(const float* hyper, int* step, float* coef, void* stream);
int avt_adam_apply_dev(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, long long n,
                       float grad_scale, const float* coef, void* stream);
/* torch.optim.SGD (maximize=False) over one flat region, with the hyper-parameters and the step count on the device as
 * in avt_adam_step_dev: hyper = device float[AVT_SGD_HYPER_FLOATS] {lr, momentum, dampening, weight_decay, nesterov
 * (0 / 1)}, read at every launch (a schedule writes it; a captured graph follows); *step = steps taken so far, read by
 * the update and incremented by a second launch behind it.  g = grad * grad_scale + weight_decay * p; with momentum:
 * buf = g at the first step (*step == 0 on entry), afterwards buf = momentum * buf + (1 - dampening) * g, then
 * g = g + momentum * buf (nesterov) or g = buf; p -= lr * g.  With momentum 0 -- or buf == NULL, which means plain SGD
 * whatever hyper[1] holds -- buf is neither read nor written.  param / grad / buf 16-byte aligned; any n >= 0. */
#define AVT_SGD_HYPER_FLOATS 5
int avt_sgd_step_dev(float* param, const float* grad, float* buf, long long n, float grad_scale, const float* hyper,
                     int* step, void* stream);
int avt_pack_conv_weight(const float* w, int K, int R, int S, int C, int Cp, int Kg, void* out_fwd, void* out_dgrad,
                         void* stream);
/* two launches (fwd copy, dgrad transpose) for many convs: descs = device array of n records
 * {const float* w; void* fwd; void* dgrad; int K, RS, C, Cp, Kg, pad;} (avt_pack_desc_bytes() each) */
size_t avt_pack_desc_bytes(void);
int avt_pack_conv_weights_batched(const void* descs, int n, long long max_elems, void* stream);
/* one of its two launches: which = 1 the fwd images, 2 the dgrad images */
int avt_pack_conv_weights_part(const void* descs, int n, long long max_elems, int which, void* stream);
/* Fold frozen BatchNorms into the convs in front of them, one launch for many convs (a whole trunk): descs = device
 * array of n records {const float* w; void* fwd; const float *gamma, *beta, *running_mean, *running_var; float* bias;
 * int K, RS, C, Cp, Kg, plain; float eps; int pad;} (avt_fold_desc_bytes() each).  With s[k] = gamma[k] *
 * rsqrt(running_var[k] + eps): fwd = the forward operand image [K][Kg] of avt_pack_conv_weights_batched holding
 * bf16(w[k,...] * s[k]) (fp32 product, one rounding; padding zero), bias[k] = beta[k] - running_mean[k] * s[k].
 * plain != 0 (the stems): fwd = the unscaled image and bias = the [2][K] (scale, shift) avt_stem_bn_relu_maxpool_fwd
 * takes.  max_elems: the largest K*Kg of the records.  Reads nothing it writes; no host sync; deterministic. */
size_t avt_fold_desc_bytes(void);
int avt_fold_conv_bn_batched(const void* descs, int n, long long max_elems, void* stream);
/* x [N][C][H][W] fp32 -> y [N][H][W][Cp] bf16 (round to nearest even, channels >= C zero).  With Cp = 4 y must be
 * 8-byte aligned, here and in avt_ncthw_to_nhwc_bf16: a pixel's four channels are stored at once. */
int avt_nchw_to_nhwc_bf16(const float* x, void* y, int N, int C, int H, int W, int Cp, void* stream);
/* x [N][C][T][H][W] fp32 -> y [(N T)][H][W][Cp] bf16: the 'b c t h w -> (b t) c h w' fold of
 * train_hardway.py:130-131 fused with the NHWC/bf16 conversion */
int avt_ncthw_to_nhwc_bf16(const float* x, void* y, int N, int C, int T, int H, int W, int Cp, void* stream);
int avt_nhwc_bf16_to_nchw(const void* x, float* y, int N, int C, int HW, void* stream);

#include "avt_tuning.h"  /* A/B knobs (process-global; not part of the drop-in path) */

#ifdef __cplusplus
}
#endif
#endif /* AVT_H_ */
