/*
 * ydl.h — C ABI of libydl_hip.so: the MI355X (gfx950) kernels behind the segmentation training hot path.
 *
 * Drop-in boundary.  The reference has no native ABI on its live path (it calls ATen through
 * nn.Module.forward); the only native interface it ships is the orphan DCNv3 pybind pair
 * (models/ops_dcnv3/src/cuda/dcnv3_cuda.h:15-31).  This header is what a reference-side binding (ctypes /
 * pybind) would bind to replace, per op, the ATen calls made by:
 *   Conv.forward            unet-lite/yolo5-seg/seg_diceloss_yolov5.py:403-409  (models/common.py:57-64)
 *   C3/C2f/SPPF/Concat      seg_diceloss_yolov5.py:416-507, yolov8/seg_jaccardloss_yolov8.py:401-414
 *   nn.Upsample / interpolate  seg_diceloss_yolov5.py:588-609, 655-657
 *   SegmentHead             segment/train.py:159-210
 *   SegmentationLoss        seg_diceloss_yolov5.py:712-750, yolov8/seg_jaccardloss_yolov8.py:774-815
 *   smart_optimizer + ModelEMA.update   utils/torch_utils.py:318-346, 404-428
 *   dcnv3_forward/backward  models/ops_dcnv3/src/cuda/dcnv3_cuda.h:15-31
 *
 * Conventions
 *  - Plain pointers and sizes only; all pointers are DEVICE pointers unless named h_*.
 *  - The caller owns every buffer (outputs, workspaces); kernels never allocate or synchronise.
 *  - Every entry point takes the HIP stream explicitly (void* = hipStream_t) and is re-entrant.
 *  - Return value: 0 on success, non-zero on error; ydl_last_error() gives a thread-local message.
 *  - Activations are NHWC: element (n,h,w,c) of a tensor with pixel stride `ld` lives at
 *    base[((n*H + h)*W + w)*ld + c].  `ld >= C`, `ld*sizeof(elem)` and `base` must be 16-byte aligned.
 *    A channel slice of a wider buffer (free concat) is just base+c0 with the wide ld.
 *  - dtype: YDL_F32 (exact-parity mode, f32 MFMA) or YDL_BF16 (throughput mode, bf16 MFMA, f32 accumulate).
 */
#ifndef YDL_H_
#define YDL_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

enum { YDL_F32 = 0, YDL_BF16 = 1, YDL_F16 = 2 /* DCNv3 op only */ };
enum { YDL_ACT_NONE = 0, YDL_ACT_SILU = 1, YDL_ACT_RELU = 2,
       YDL_ACT_LEAKY = 3 /* z > 0 ? z : slope * z; the slope is the act_param of the *_p entry points, 0 <= slope < 1 */,
       YDL_ACT_HSWISH = 4 /* z * relu6(z + 3) / 6 */, YDL_ACT_MISH = 5 /* z * tanh(softplus(z)) */ };
/* residual handling of the fused BN/activation kernels */
enum { YDL_RES_NONE = 0, YDL_RES_AFTER_ACT = 1 /* C3/C2f: act(bn(y)) + r */, YDL_RES_BEFORE_ACT = 2 /* ResNet: act(bn(y) + r) */,
       YDL_RES_GRAD_ACCUMULATE = 16 /* ydl_bn_act_bwd only, or-ed into res_mode: dres += instead of dres = */ };
enum { YDL_LOSS_DICE = 0, YDL_LOSS_JACCARD = 1 };

const char* ydl_last_error(void);
int ydl_version(void);
/* Test-only, process-wide debug knobs for A/B tests (key 0: bf16 wgrad operand path, 1: streaming point-wise kernel on/off,
 * 2: strided dgrad in one launch / per class).  They change launch geometry: a caller that caches ydl_conv_fwd_grid_m /
 * _block_m / _stats_ws_bytes must drop its cache after a change.  Everything else in the library is per call or per
 * device (kernel attributes and the CU count are keyed by the HIP device id current at the call). */
void ydl_debug_set(int key, int val);
/* diagnostics: number of (kernel, device) launch-attribute initialisations done so far */
int ydl_debug_attr_sets(void);
/* diagnostics: name of the kernel instantiation the last call of an entry family launched (process-wide);
 * family 0 ydl_conv_fwd, 1 ydl_conv_dgrad, 2 ydl_conv_wgrad, 3 ydl_bn_finalize, 4 ydl_deform_bwd, 5 ydl_deform_gather,
 * 6 ydl_conv_bwd_pw_bn (which also sets 1 and 2, as ydl_conv_bwd_pw does: the kernel is the same pwbw_kernel).
 * "" if none yet. */
const char* ydl_debug_last_kernel(int family);

/* ---- convolution as implicit GEMM on MFMA ------------------------------------------------------------
 * Geometry of one conv layer (square kernel k, stride s, padding p, groups=1, no bias).
 * Weights in compute layout: w  = [Cout][k*k][Cin_p]   (KRSC; Cin_p = Cin rounded up to 8)
 *                            wt = [Cin][k*k][Cout_p]   (transposed, for dgrad; Cout_p = Cout rounded up to 8)
 */
typedef struct {
    int N, Hi, Wi, Cin;       /* input  (Cin = logical channels; reads Cin_p = round_up(Cin, 8) <= ldx) */
    int Ho, Wo, Cout;         /* output */
    int k, s, p;
    int ldx, ldy;             /* pixel strides of x and y (elements) */
    int ldw;                  /* row stride (elements) of w in conv_fwd and of dw in conv_wgrad; 0 = dense = k*k*Cin_p.
                                 A larger stride addresses a COLUMN BLOCK of a wider 1x1 weight matrix: a convolution
                                 over a channel concat is evaluated as the sum of one convolution per source */
} ydl_conv_geom;

/* BN-statistics workspace of the forward epilogue: [grid_m][2][round_up(Cout,8)] floats of (sum, M2) per channel, row b for
 * block b of the launch.  A block is one launch tile, which may be a 2-D patch of the image: only the row count grid_m and the
 * per-row pixel count min(block_m, N*Ho*Wo - b*block_m) are promised, not which pixels a row covers.  The workspace also holds
 * the room ydl_bn_finalize needs behind the rows.  The three queries are pure functions of g (and of the debug knobs), run on
 * the host without a device, and describe the launch ydl_conv_fwd makes with stats_ws != NULL and accumulate == 0 (a launch that
 * accumulates on a geometry where they would differ returns an error); 0 for a geometry ydl_conv_fwd refuses. */
int64_t ydl_conv_fwd_stats_ws_bytes(const ydl_conv_geom* g, int dtype);
int ydl_conv_fwd_grid_m(const ydl_conv_geom* g, int dtype);
int ydl_conv_fwd_block_m(const ydl_conv_geom* g, int dtype);

/* y (+)= conv(x, w).  If stats_ws != NULL the epilogue also writes per-block (sum, M2) partials of the values it
 * stores (f32 accumulators, plus the previous contents of y when accumulate != 0) per output channel for train-mode
 * BN; finish them with ydl_bn_finalize. */
int ydl_conv_fwd(const ydl_conv_geom* g, int dtype, const void* x, const void* w, void* y,
                 float* stats_ws, int accumulate, void* stream);
/* dx (+)= conv_transpose(dy, wt).  accumulate != 0 adds into dx (gradient fan-in).
 * The same three entry points run nn.ConvTranspose2d(c1, c2, k, 2, p, op) with the roles of x and dy exchanged, on the MIRRORED
 * geometry {N, Hi = 2H, Wi = 2W, Cin = c2, Ho = H, Wo = W, Cout = c1, k, 2, p, ldx = ld of y / dy, ldy = ld of x}: the parameter
 * [c1][c2][k][k] in channels_last storage is the KRSC master [c1][k*k][c2] of that convolution (ydl_weight_prep(master, w, wt, c1,
 * k*k, c2)); forward y = ydl_conv_dgrad(dy := x, wt, dx := y), input gradient ydl_conv_fwd(x := dy, w, y := dx), weight gradient
 * ydl_conv_wgrad(x := dy, dy := x).  (k, p, op) in {(2,0,0), (4,1,0), (3,1,1)} give Hi = 2H exactly. */
int ydl_conv_dgrad(const ydl_conv_geom* g, int dtype, const void* dy, const void* wt, void* dx,
                   int accumulate, void* stream);
/* Input gradient AND weight gradient of a 1x1 / stride-1 convolution in ONE pass over dy (both are HBM-bound on large maps: dy is
 * fetched once instead of twice; csrc/igemm.hip: pwbw_kernel).  Supported (ydl_conv_bwd_pw_supported != 0): bf16, Cin = Cout = 128,
 * at least 131 072 pixels.  dx has its own pixel stride lddx (a channel slice of a wider gradient buffer); accumulate != 0 adds into
 * dx; dw[Cout][g->ldw or 128] receives f32 atomic adds like ydl_conv_wgrad.  wt = [128][128] (ydl_conv_dgrad's operand). */
int ydl_conv_bwd_pw_supported(const ydl_conv_geom* g, int dtype);
int ydl_conv_bwd_pw(const ydl_conv_geom* g, int dtype, const void* x, const void* dy, const void* wt, void* dx, int lddx,
                    int accumulate, float* dw, void* stream);
/* ydl_conv_bwd_pw for a layer whose dy is the result of a BatchNorm backward that nobody else reads: the kernel takes what the
 * apply pass of ydl_bn_act_bwd_sums takes — the saved pre-activation y (pixel stride ldy), dout, the four coefficient rows, the
 * COMPLETED replica sums (ydl_bn_act_bwd_reduce_sums has ended) — and forms dy = scale * (dz - sum dz / npix - xhat * sum dz xhat /
 * npix) itself while the tiles arrive, bit for bit what the apply pass stores; that launch and its three tensor passes disappear
 * (csrc/igemm.hip: pwbw_kernel<S, ACC, BN>; ydl_debug_last_kernel(6) names the instantiation).  Same geometries as ydl_conv_bwd_pw.  dout is ONE segment of 128 channels (dout1 = sums1 = NULL,
 * sums0 = [YDL_BN_REPLICAS][2][128]) or TWO segments of 64 channels with pixel strides of their own and sums0 / sums1 =
 * [YDL_BN_REPLICAS][2][64] each (a fused sibling pair activates its halves into two places; both segments must lie within 4 GiB of
 * each other); mean / invstd / scale / shift / dgamma / dbeta are rows of 128.  act: YDL_ACT_NONE or YDL_ACT_SILU.  Block 0 stores
 * (or, accumulate_param_grads != 0, adds) dgamma / dbeta as the apply pass does.  dy_out (optional, pixel stride lddy) also
 * receives dy, for a second reader.  x, wt, dx, lddx, accumulate, dw: as ydl_conv_bwd_pw. */
int ydl_conv_bwd_pw_bn_supported(const ydl_conv_geom* g, int dtype);
int ydl_conv_bwd_pw_bn(const ydl_conv_geom* g, int dtype, const void* x, const void* y, int ldy, const void* dout0, int lddo0,
                       const void* dout1, int lddo1, const float* mean, const float* invstd, const float* scale, const float* shift,
                       const float* sums0, const float* sums1, int64_t npix, int act, float* dgamma, float* dbeta,
                       int accumulate_param_grads, void* dy_out, int lddy, const void* wt, void* dx, int lddx, int accumulate,
                       float* dw, void* stream);
/* The input gradient with the BatchNorm backward's REDUCE pass of the layer(s) that produced the convolution's input fused into
 * its epilogue (throughput mode: replica sums, see ydl_bn_act_bwd_sums).  dx — the gradient this call completes, i.e. the `dout` of
 * those layers — is still in registers when it is stored: the epilogue reads the producers' saved pre-activations y once,
 * forms dz = dx * act'(y*scale + shift) and adds (sum dz, sum dz*xhat) per channel into sums[i] = [YDL_BN_REPLICAS][2][cp[i]]
 * (zeroed by the caller), so ydl_bn_act_bwd_apply_sums can follow without the reduce launch and its second read of dx.
 * Valid only when this call is the LAST writer of dx (accumulate != 0 is fine: the stored sum is what is reduced).
 * Up to two channel segments [c0, c1) of dx (multiples of 8), each with its own producer: a channel concat of two layers.
 * Per-segment pointers are at the segment's channel 0 (= channel c0 of dx).  act: YDL_ACT_NONE or YDL_ACT_SILU.
 * ydl_conv_dgrad_bnred_supported: 1 when this geometry runs on a kernel whose epilogue has the fused form (bf16 ring kernels),
 * else use ydl_conv_dgrad + ydl_bn_act_bwd_sums. */
typedef struct {
    int nseg;
    int c0[2], c1[2], ldy[2], cp[2], act[2];
    const void* y[2];
    const float* scale[2];
    const float* shift[2];
    const float* mean[2];
    const float* invstd[2];
    float* sums[2];
} ydl_bnred;
int ydl_conv_dgrad_bnred_supported(const ydl_conv_geom* g, int dtype);
int ydl_conv_dgrad_bnred(const ydl_conv_geom* g, int dtype, const void* dy, const void* wt, void* dx,
                         int accumulate, const ydl_bnred* red, void* stream);
/* dw[Cout][k*k][Cin_p] (f32) += sum over pixels dy^T * im2col(x).  dw must be zeroed (or hold the running
 * sum for gradient accumulation) before the call: split-K blocks add with f32 atomics. */
int ydl_conv_wgrad(const ydl_conv_geom* g, int dtype, const void* x, const void* dy, float* dw, void* stream);
/* Deterministic form (bitwise reproducible from run to run): every split-K block stores its partial tile into
 * ws = [splits][Cout][k*k*Cin_p] f32 (ydl_conv_wgrad_ws_bytes) and a second kernel adds the partials into dw in a fixed
 * order.  Same products and tiles as ydl_conv_wgrad; parity mode (YDL_F32) uses it by default. */
int64_t ydl_conv_wgrad_ws_bytes(const ydl_conv_geom* g, int dtype);
int ydl_conv_wgrad_det(const ydl_conv_geom* g, int dtype, const void* x, const void* dy, float* dw, float* ws, void* stream);

/* Throughput-mode statistics: the same convolution, but every block ADDS its per-channel (sum, sum of squares) with f32 atomics
 * into sums = [YDL_BN_REPLICAS][2][round_up(Cout,8)] floats (replica = block index mod YDL_BN_REPLICAS, which spreads the
 * contention; the caller zeroes the buffer) instead of writing a partial row: no ydl_bn_finalize launch — ydl_bn_act_fwd_sums
 * derives the coefficients from the sums itself.  The sums depend on arrival order in their last bits (run-to-run differences
 * of 1e-7 relative in mean / variance): parity mode keeps the deterministic partial rows + ydl_bn_finalize. */
#define YDL_BN_REPLICAS 8
int ydl_conv_fwd_sums(const ydl_conv_geom* g, int dtype, const void* x, const void* w, void* y,
                      float* sums, int accumulate, void* stream);

/* master weights (f32, KRSC [Cout][k*k][Cin]) -> compute copies: w [Cout][kk][Cin_p] and wt [Cin][kk][Cout_p] */
int ydl_weight_prep(int dtype, const float* master, void* w, void* wt, int Cout, int kk, int Cin, void* stream);
/* the same for every layer of a model in one launch; desc_dev: device array of nlayers x 8 int64
 * {master*, w*, wt*, Cout, kk, Cin, 0, 0} */
int ydl_weight_prep_batched(int dtype, const int64_t* desc_dev, int nlayers, void* stream);
/* dw [Cout][kk][Cin_p] f32 -> master-layout grad [Cout][kk][Cin] (only needed when Cin_p != Cin) */
int ydl_wgrad_unpad(const float* dw, float* grad, int Cout, int kk, int Cin, int accumulate, void* stream);

/* ---- grouped convolution, 1 < groups < channels (csrc/gconv.hip) -----------------------------------
 * nn.Conv2d(Cin, Cout, k, 1, k/2, groups=groups, bias=False) on the same ydl_conv_geom (Cin, Cout: the WHOLE tensors' channels):
 * output channel c reads the input channels of group c / (Cout/groups) only.  ONE launch serves every group.
 * Served set (ydl_gconv_supported != 0; everything else returns an error): groups >= 2, Cin/groups and Cout/groups multiples
 * of 16, k in {1, 3}, s = 1, p = k/2, ldw = 0, pixel strides as for ydl_conv_fwd.  x, y, dy, dx may be channel slices of wider
 * buffers (ldx / ldy larger than the channel count); channels outside the slice are never written.  f32 accumulation, no atomics:
 * the same kernels serve throughput mode and deterministic mode, and every result is bitwise reproducible.
 * Weights: w  = [Cout][k*k][Cin/groups]  (the KRSC master shape: nn.Conv2d(groups).weight in channels_last storage)
 *          wt = [Cin][k*k][Cout/groups]  (per-group transpose, for the input gradient). */
int ydl_gconv_supported(const ydl_conv_geom* g, int groups, int dtype);
/* master (f32, w's shape) -> compute-dtype copies w and wt, one launch */
int ydl_gconv_weight_prep(int dtype, const float* master, void* w, void* wt, int Cout, int kk, int Cin, int groups, void* stream);
/* y = gconv(x, w).  stats_ws != NULL: also writes per-block (sum, M2) rows of the STORED output, [rows][2][round_up(Cout,8)] floats
 * with rows = ceil(N*Ho*Wo / block_m), row b covering pixels [b*block_m, (b+1)*block_m), in the format ydl_bn_finalize consumes.
 * ydl_gconv_fwd_block_m / _stats_ws_bytes are pure host functions of the geometry (0 for a geometry outside the served set); the
 * workspace size includes the room ydl_bn_finalize needs behind the rows. */
int ydl_gconv_fwd_block_m(const ydl_conv_geom* g, int groups, int dtype);
int64_t ydl_gconv_fwd_stats_ws_bytes(const ydl_conv_geom* g, int groups, int dtype);
int ydl_gconv_fwd(const ydl_conv_geom* g, int groups, int dtype, const void* x, const void* w, void* y, float* stats_ws, void* stream);
/* dx (+)= gconv_transpose(dy, wt).  accumulate != 0 adds into dx. */
int ydl_gconv_dgrad(const ydl_conv_geom* g, int groups, int dtype, const void* dy, const void* wt, void* dx, int accumulate,
                    void* stream);
/* dw [Cout][k*k][Cin/groups] (f32, the master gradient's layout) += sum over pixels dy^T * im2col(x).  Every block stores its
 * partial tile into ws (ydl_gconv_wgrad_ws_bytes, a pure host function) and a second kernel adds the partials into dw in a
 * fixed order: bitwise reproducible.  dw holds zeros or the running sum of gradient accumulation. */
int64_t ydl_gconv_wgrad_ws_bytes(const ydl_conv_geom* g, int groups, int dtype);
int ydl_gconv_wgrad(const ydl_conv_geom* g, int groups, int dtype, const void* x, const void* dy, float* dw, float* ws, void* stream);

/* ---- cross convolution: k taps along ONE image axis (csrc/xconv.hip) -------------------------------
 * YDL_AXIS_W: nn.Conv2d(Cin, Cout, (1,k), (1,s), (0,p), bias=False);  YDL_AXIS_H: nn.Conv2d(Cin, Cout, (k,1), (s,1), (p,0), bias=False)
 * — the two convolutions of CrossConv (models/common.py:147-158) — on the same ydl_conv_geom: k, s and p apply along the named axis;
 * along the other axis the kernel is 1, the stride 1 and the padding 0, so Ho = Hi (W) or Wo = Wi (H).
 * Served set (ydl_xconv_supported != 0; everything else returns an error that names the failing condition, on the host, before
 * anything is enqueued): k odd with 3 <= k <= 9, s in {1, 2}, p = k/2, Cin and Cout multiples of 8, ldw = 0, output size
 * (L + 2p - k)/s + 1 along the axis, pixel strides as for ydl_conv_fwd.  x, y, dy, dx may be channel slices of wider buffers;
 * channels outside the slice are never read into a result and never written.  f32 accumulation, no atomics: the same launches
 * serve throughput mode and deterministic mode, and every result is bitwise reproducible.
 * Weights: the KRSC master [Cout][k][Cin] is nn.Conv2d(...).weight in channels_last storage for BOTH orientations; the compute
 * copies w = [Cout][k][Cin] and wt = [Cin][k][Cout] come from ydl_weight_prep with kk = k. */
enum { YDL_AXIS_W = 0, YDL_AXIS_H = 1 };
int ydl_xconv_supported(const ydl_conv_geom* g, int axis, int dtype);
/* y = xconv(x, w).  stats_ws != NULL: also writes per-block (sum, M2) rows of the STORED output, [rows][2][Cout] floats with
 * rows = ceil(N*Ho*Wo / block_m), row b covering pixels [b*block_m, (b+1)*block_m), in the format ydl_bn_finalize consumes.
 * ydl_xconv_fwd_block_m / _stats_ws_bytes are pure host functions of the geometry (0 outside the served set); the workspace size
 * includes the room ydl_bn_finalize needs behind the rows. */
int ydl_xconv_fwd_block_m(const ydl_conv_geom* g, int axis, int dtype);
int64_t ydl_xconv_fwd_stats_ws_bytes(const ydl_conv_geom* g, int axis, int dtype);
int ydl_xconv_fwd(const ydl_conv_geom* g, int axis, int dtype, const void* x, const void* w, void* y, float* stats_ws, void* stream);
/* dx (+)= xconv_transpose(dy, wt); at stride 2 a gather over the exact quotients (i + p - t)/2.  accumulate != 0 adds into dx. */
int ydl_xconv_dgrad(const ydl_conv_geom* g, int axis, int dtype, const void* dy, const void* wt, void* dx, int accumulate,
                    void* stream);
/* dw [Cout][k][Cin] (f32, the master gradient's layout) += sum over pixels dy^T * shifted x.  Every block stores its partial tile
 * into ws (ydl_xconv_wgrad_ws_bytes, a pure host function: the split count depends on the geometry alone) and a second kernel adds
 * the partials into dw in a fixed order: bitwise reproducible.  dw holds zeros or the running sum of gradient accumulation. */
int64_t ydl_xconv_wgrad_ws_bytes(const ydl_conv_geom* g, int axis, int dtype);
int ydl_xconv_wgrad(const ydl_conv_geom* g, int axis, int dtype, const void* x, const void* dy, float* dw, float* ws, void* stream);

/* ---- train-mode BatchNorm + activation ------------------------------------------------------------- */
/* Chan-merge the per-block partials; writes mean/invstd (saved for backward), scale=gamma*invstd,
 * shift=beta-mean*scale; updates running_mean/var (momentum, unbiased var) and is a no-op on them if NULL. */
int ydl_bn_finalize(const float* stats_ws, int nblocks, int block_m, int64_t count, int C,
                    const float* gamma, const float* beta,
                    float eps, float momentum, float* running_mean, float* running_var,
                    float* mean, float* invstd, float* scale, float* shift,
                    int replication /* >=1: the logical tensor is the stored one nearest-replicated this many times
                                       (lazy up-sampling); only the unbiased running_var factor depends on it */,
                    void* stream);
/* eval-mode: scale/shift from running statistics */
int ydl_bn_eval_coeffs(int C, const float* gamma, const float* beta, const float* running_mean,
                       const float* running_var, float eps, float* scale, float* shift, void* stream);
/* out = act(y*scale+shift) [+ res] ; res_mode per YDL_RES_*.  Cp = channels processed (multiple of 8). */
int ydl_bn_act_fwd(int dtype, const void* y, int ldy, const float* scale, const float* shift,
                   const void* res, int ldr, int res_mode, int act, void* out, int ldo,
                   int64_t npix, int Cp, void* stream);
int64_t ydl_bn_bwd_ws_bytes(int64_t npix, int Cp);
/* Backward of out = act(bn(y)) [+res].  dout: grad wrt out.  out: saved output (needed only for RELU).
 * Writes dy (grad wrt conv output), dgamma/dbeta (f32, accumulate flag) and, when dres is not NULL, the gradient of the residual
 * branch in the same pass: the masked gradient dz for YDL_RES_BEFORE_ACT, dout itself for YDL_RES_AFTER_ACT; res_mode may carry
 * YDL_RES_GRAD_ACCUMULATE (dres already holds another consumer's gradient: add to it). */
int ydl_bn_act_bwd(int dtype, const void* y, int ldy, const void* dout, int lddo, const void* out, int ldo,
                   const float* gamma, const float* mean, const float* invstd, const float* scale, const float* shift,
                   int res_mode, int act, void* dy, int lddy, void* dres, int lddr,
                   float* dgamma, float* dbeta, int accumulate_param_grads,
                   float* ws, int64_t npix, int C, int Cp, void* stream);

/* The two-launch forms on replica sums (throughput mode; see ydl_conv_fwd_sums).
 * ydl_bn_act_fwd_sums = ydl_bn_finalize + ydl_bn_act_fwd in ONE launch: every thread derives mean / invstd / scale / shift of its
 * channel chunk from sums = [YDL_BN_REPLICAS][2][sums_ld] (count = pixels the sums cover), block 0 also stores them (mean, invstd,
 * scale, shift: [Cp] each, read again by the backward) and updates the running statistics.  All per-channel pointers and `sums`
 * may point INTO wider arrays (a channel group of a fused sibling convolution): sums_ld is the row stride of the sums.
 * ydl_bn_act_bwd_sums = ydl_bn_act_bwd without its merge launch: the reduce pass adds (sum dz, sum dz*xhat) into
 * sums = [YDL_BN_REPLICAS][2][Cp] (zeroed by the caller), the apply pass reads them; block 0 of the apply pass stores or adds
 * dgamma / dbeta. */
int ydl_bn_act_fwd_sums(int dtype, const void* y, int ldy, const float* sums, int sums_ld, int64_t count,
                        const float* gamma, const float* beta, float eps, float momentum,
                        float* running_mean, float* running_var, float* mean, float* invstd, float* scale, float* shift,
                        int replication, const void* res, int ldr, int res_mode, int act, void* out, int ldo,
                        int64_t npix, int C, int Cp, void* stream);
int ydl_bn_act_bwd_sums(int dtype, const void* y, int ldy, const void* dout, int lddo, const void* out, int ldo,
                        const float* mean, const float* invstd, const float* scale, const float* shift,
                        int res_mode, int act, void* dy, int lddy, void* dres, int lddr,
                        float* dgamma, float* dbeta, int accumulate_param_grads,
                        float* sums, int64_t npix, int C, int Cp, void* stream);
/* the apply pass alone: sums already hold (sum dz, sum dz*xhat) of this tensor (ydl_conv_dgrad_bnred) */
int ydl_bn_act_bwd_apply_sums(int dtype, const void* y, int ldy, const void* dout, int lddo, const void* out, int ldo,
                              const float* mean, const float* invstd, const float* scale, const float* shift,
                              int res_mode, int act, void* dy, int lddy, void* dres, int lddr,
                              float* dgamma, float* dbeta, int accumulate_param_grads,
                              float* sums, int64_t npix, int C, int Cp, void* stream);
/* the reduce pass alone, for a layer whose consumer forms dy itself (ydl_conv_bwd_pw_bn): adds (sum dz, sum dz*xhat) into the zeroed
 * sums and writes (res_mode & YDL_RES_GRAD_ACCUMULATE: adds) the gradient of the residual operand into dres, as the apply pass would
 * have; dgamma / dbeta are left to the consumer, because the sums are complete only when this kernel has ended */
int ydl_bn_act_bwd_reduce_sums(int dtype, const void* y, int ldy, const void* dout, int lddo, const void* out, int ldo,
                               const float* mean, const float* invstd, const float* scale, const float* shift,
                               int res_mode, int act, void* dres, int lddr, float* sums, int64_t npix, int C, int Cp, void* stream);

/* ---- spatial ops (NHWC, channel-vectorised) -------------------------------------------------------- */
/* The pixel tensors of this section (x, y, dy, dx, a, b; not the per-image rows avg / max / davg / dmax and not gate) are read and
 * written as 16-byte channel vectors: their pointers must be 16-byte aligned and their pixel strides whole chunks (4 f32 / 8 bf16
 * elements), or the call is refused without a launch.  ydl_copy2d alone serves any alignment (an element-granular kernel). */
/* max pool (k,s,p), -inf padding; idx (uint8 window offset of the arg-max, first max in scan order) is
 * written when non-NULL and consumed by the backward. */
int ydl_maxpool_fwd(int dtype, const void* x, int ldx, void* y, int ldy, uint8_t* idx,
                    int N, int Hi, int Wi, int Ho, int Wo, int C, int k, int s, int p, void* stream);
int ydl_maxpool_bwd(int dtype, const void* dy, int lddy, const uint8_t* idx, void* dx, int lddx, int accumulate,
                    int N, int Hi, int Wi, int Ho, int Wo, int C, int k, int s, int p, void* stream);
/* SPPF's chain of three k x k / stride 1 / pad k/2 max-pools (y1 = mp(x), y2 = mp(y1), y3 = mp(y2); seg_diceloss_yolov5.py:468-481,
 * models/common.py:223-238) in one launch per direction, the H x W plane held in LDS: same values, index planes and gradients as
 * three ydl_maxpool_fwd / ydl_maxpool_bwd calls, bit for bit.  ydl_sppf_pool_supported: 1 when the plane fits (else use those).
 * Backward: dyK = gradient already present in the slice of yK (the concat consumer's input gradient), dx (+)= the chain's result. */
int ydl_sppf_pool_supported(int dtype, int H, int W, int C, int k);
int ydl_sppf_pool_fwd(int dtype, const void* x, int ldx, void* y1, void* y2, void* y3, int ldy,
                      uint8_t* idx1, uint8_t* idx2, uint8_t* idx3, int N, int H, int W, int C, int k, void* stream);
int ydl_sppf_pool_bwd(int dtype, const void* dy1, const void* dy2, const void* dy3, int lddy, const uint8_t* idx1,
                      const uint8_t* idx2, const uint8_t* idx3, void* dx, int lddx, int accumulate,
                      int N, int H, int W, int C, int k, void* stream);
/* The parallel pyramid of SPP / C3SPP / SPPCSPC (models/common.py:1282-1286, :1439-1446): yi = max-pool(x; ki, stride 1, pad ki/2),
 * all three of the same x, in one launch per direction, the H x W plane held in LDS.  ki odd, 3..15, any order.  Same values,
 * index planes and dx as ydl_maxpool_fwd(x -> yi, ki, 1, ki/2) three times and ydl_maxpool_bwd(dy1, idx1, accumulate), (dy2, idx2, 1),
 * (dy3, idx3, 1), bit for bit; the backward is a gather without atomics.  ydl_spp_pool_supported: 1 when the window sizes are
 * served and the plane fits (else use those calls); the other two return an error without launching when it is 0. */
int ydl_spp_pool_supported(int dtype, int H, int W, int C, int k1, int k2, int k3);
int ydl_spp_pool_fwd(int dtype, const void* x, int ldx, void* y1, void* y2, void* y3, int ldy,
                     uint8_t* idx1, uint8_t* idx2, uint8_t* idx3, int N, int H, int W, int C, int k1, int k2, int k3, void* stream);
int ydl_spp_pool_bwd(int dtype, const void* dy1, const void* dy2, const void* dy3, int lddy, const uint8_t* idx1,
                     const uint8_t* idx2, const uint8_t* idx3, void* dx, int lddx, int accumulate,
                     int N, int H, int W, int C, int k1, int k2, int k3, void* stream);
/* resize: mode 0 nearest (src=min(floor(dst*scale),in-1)), 1 bilinear align_corners=False, 2 bilinear
 * align_corners=True.  scale_h/w <= 0 means "derive from sizes" (in/out, or (in-1)/(out-1)).  Modes 3 and 4 (the tape's
 * RESIZE_BICUBIC / RESIZE_BICUBIC_AC) are refused here with a message: bicubic has the entry points ydl_bicubic_fwd / _bwd below. */
int ydl_resize_fwd(int dtype, int mode, const void* x, int ldx, void* y, int ldy,
                   int N, int Hi, int Wi, int Ho, int Wo, int C, float scale_h, float scale_w, void* stream);
int ydl_resize_bwd(int dtype, int mode, const void* dy, int lddy, void* dx, int lddx, int accumulate,
                   int N, int Hi, int Wi, int Ho, int Wo, int C, float scale_h, float scale_w, void* stream);
/* bicubic resize, ATen's upsample_bicubic2d (A = -0.75); align != 0 is align_corners=True.  scale as above.  src = scale*(dst+0.5)-0.5
 * NOT clamped at 0 (align: scale*dst), i = floor(src), t = src - i, taps i-1 .. i+2 each clamped to [0, in-1], coefficients
 * c0 = ((A(t+1) - 5A)(t+1) + 8A)(t+1) - 4A, c1 = ((A+2)t - (A+3))t*t + 1, c2 = c1 at 1-t, c3 = c0's cubic at (1-t)+1, all in
 * round-to-nearest f32 operations; the output is the separable 4 x 4 sum in f32.  The backward is the exact transpose in gather form
 * (no atomics, bitwise reproducible); accumulate != 0 adds into dx. */
int ydl_bicubic_fwd(int dtype, int align, const void* x, int ldx, void* y, int ldy,
                    int N, int Hi, int Wi, int Ho, int Wo, int C, float scale_h, float scale_w, void* stream);
int ydl_bicubic_bwd(int dtype, int align, const void* dy, int lddy, void* dx, int lddx, int accumulate,
                    int N, int Hi, int Wi, int Ho, int Wo, int C, float scale_h, float scale_w, void* stream);
/* y += resize(x) (same modes and index arithmetic as ydl_resize_fwd); with ``sums`` != NULL also adds the per-channel (sum, sum of
 * squares) of the result to BatchNorm replica rows sums[YDL_BN_REPLICAS][2][sums_ld], exactly like ydl_conv_fwd_sums' epilogues: the
 * last launch of a 1x1 Conv over the auto-aligned Concat [a, resize(b)] (seg_diceloss_yolov5.py:484-507 + :388-409) evaluated as
 * conv_a(a) + resize(conv_b(b)) */
int ydl_resize_acc_sums(int dtype, int mode, const void* x, int ldx, void* y, int ldy, int N, int Hi, int Wi, int Ho, int Wo,
                        int C, float scale_h, float scale_w, float* sums, int sums_ld, void* stream);
/* strided channel-slice copy / add:  dst[:, 0:C] (op)= src[:, 0:C] */
int ydl_copy2d(int dtype, const void* src, int lds, void* dst, int ldd, int64_t npix, int C, int accumulate,
               void* stream);
/* layout/dtype conversion at the model edge: NCHW f32 <-> NHWC compute dtype (channels padded with zeros) */
int ydl_nchw_to_nhwc(int dtype, const float* src, void* dst, int ldd, int N, int C, int H, int W, void* stream);
/* space-to-depth edge conversion for a stem conv with k % s == 0 and p % s == 0 (seg_diceloss_yolov5.py backbone layer 0:
 * Conv(3, 64, 6, 2, 2)):  conv(k,s,p) on (H,W,C) == conv(k/s,1,p/s) on (H/s, W/s, s*s*C), channel (dy*s+dx)*C + c.
 * ydl_weight_prep_s2d / ydl_wgrad_unpack_s2d apply the same index map to the KRSC weight and its gradient. */
int ydl_nchw_to_s2d(int dtype, const float* src, void* dst, int ldd, int N, int C, int H, int W, int s, void* stream);
/* space-to-depth / depth-to-space on interior NHWC tensors (Focus, Contract, Expand: models/common.py:241-250, :282-307); each is the
 * other's backward.  Rows are NHWC with strides ldx / ldy in elements.
 *   ydl_space_to_depth: x (N, H, W, C)     -> y (N, H/s, W/s, s*s*C):  y[n, ho, wo, blk(sy,sx)*C + c] (+)= x[n, ho*s+sy, wo*s+sx, c]
 *   ydl_depth_to_space: x (N, H, W, s*s*C) -> y (N, H*s, W*s, C):      y[n, h*s+sy, w*s+sx, c] (+)= x[n, h, w, blk(sy,sx)*C + c]
 * order 0: blk = sy*s + sx (Contract, Expand, ydl_nchw_to_s2d); order 1: blk = sx*s + sy (Focus's concat order).  Only the channels
 * [0, s*s*C) / [0, C) of each output row are written.  accumulate != 0 adds in f32 with one rounding.  No atomics.  16-byte chunks move
 * when C, both strides and both pointers are whole chunks; an element-granular kernel serves every other alignment.  Refused: H or W
 * not a multiple of s (space-to-depth), a stride shorter than its row, s < 1, order outside {0, 1}. */
int ydl_space_to_depth(int dtype, const void* x, int ldx, void* y, int ldy, int N, int H, int W, int C, int s, int order,
                       int accumulate, void* stream);
int ydl_depth_to_space(int dtype, const void* x, int ldx, void* y, int ldy, int N, int H, int W, int C, int s, int order,
                       int accumulate, void* stream);
int ydl_weight_prep_s2d(int dtype, const float* master, void* w2, int Cout, int k, int s, int C, void* stream);
int ydl_wgrad_unpack_s2d(const float* dw2, float* grad, int Cout, int k, int s, int C, int accumulate, void* stream);
int ydl_nhwc_to_nchw(int dtype, const void* src, int lds, float* dst, int N, int C, int H, int W, int accumulate,
                     void* stream);
/* generic elementwise on NHWC slices: out = a * b_bcast ... used by GAM (x * gate[n,c]) */
int ydl_scale_channels(int dtype, const void* x, int ldx, const float* gate /*[N][C]*/, void* y, int ldy,
                       int N, int64_t hw, int C, void* stream);

/* GAM (unet-lite/yolo9-seg/seg_diceloss_yolov9.py:475-510): global average / max pooling to 1x1 (argmax = pixel index of the
 * first maximum -- a NaN wins and the last NaN stays, as in ATen's scan --, int32 [N][C rounded up to a 16-byte chunk of the
 * dtype]; avg and max are written for that many channels), sigmoid gate of two pooled branches, per-(n,c) dot product */
int ydl_global_pool_fwd(int dtype, const void* x, int ldx, void* avg, int lda, void* mx, int ldm, int32_t* argmax,
                        int N, int64_t HW, int C, void* stream);
int ydl_global_pool_bwd(int dtype, const void* davg, int lda, const void* dmx, int ldm, const int32_t* argmax,
                        void* dx, int lddx, int accumulate, int N, int64_t HW, int C, void* stream);
int ydl_gate_fwd(int dtype, const void* a, int lda, const void* b, int ldb, float* gate, int N, int C, void* stream);
int ydl_gate_bwd(int dtype, const float* gate, const float* dgate, void* da, int lda, int acc_a, void* db, int ldb,
                 int acc_b, int N, int C, void* stream);
int ydl_channel_dot(int dtype, const void* a, int lda, const void* b, int ldb, float* out, int N, int64_t HW, int C,
                    void* stream);

/* ---- softmax over channels (the yaml models end in nn.Softmax(1)) ----------------------------------- */
/* x: NHWC compute dtype (C<=32), stored at (H, W); p: f32 of logical size (N, C, H*rep_h, W*rep_w) with element
 * strides (sn, sc, sh, sw) — NCHW or NHWC.  rep_* > 1 fuses a nearest up-sampling of the probabilities. */
int ydl_softmax_fwd(int dtype, const void* x, int ldx, float* p, int64_t sn, int64_t sc, int64_t sh, int64_t sw,
                    int N, int H, int W, int C, int rep_h, int rep_w, void* stream);
/* dx = p * (dps - sum_c p*dps), dps = dp summed over the rep_h x rep_w replicas of each stored pixel */
int ydl_softmax_bwd(int dtype, const float* p, const float* dp, int64_t sn, int64_t sc, int64_t sh, int64_t sw,
                    void* dx, int lddx, int N, int H, int W, int C, int rep_h, int rep_w, void* stream);

/* ---- CE + 0.5*(Dice|Jaccard) loss ------------------------------------------------------------------ */
/* ws layout (f32): see ydl_seg_loss_ws_floats.  losses[0..2] = total, ce, overlap-loss (device, no sync). */
int64_t ydl_seg_loss_ws_floats(int N, int C);
int ydl_seg_loss_fwd(const float* pred, int64_t sn, int64_t sc, int64_t sh, int64_t sw,
                     const int64_t* target, int Ht, int Wt, const float* class_weights /* NULL = ones */,
                     int kind, float label_smoothing, float eps, int N, int C, int H, int W,
                     float* ws, float* losses, void* stream);
/* dpred = dloss * dL/dpred, using the sums left in ws by the forward */
int ydl_seg_loss_bwd(const float* pred, int64_t sn, int64_t sc, int64_t sh, int64_t sw,
                     const int64_t* target, int Ht, int Wt, const float* class_weights,
                     int kind, float label_smoothing, float eps, int N, int C, int H, int W,
                     const float* ws, const float* dloss /* device scalar, NULL = 1 */, float* dpred, void* stream);

/* Replicated-prediction variant of the two calls above: the (N, C, H*rep_h, W*rep_w) prediction is the exact nearest
 * replication of `plow` (N, C, H, W) — the lazily evaluated `Upsample(nearest) -> Conv 1x1 -> Softmax` tail of the yaml
 * models (seg_diceloss_yolov5.py:588-614 builds it).  target is (N, H*rep_h, W*rep_w) int64.  Same ws layout, same
 * `losses`; the backward returns dlow[n,c,h,w] = sum over the rep_h*rep_w replicas of d loss / d pred. */
int ydl_seg_loss_rep_fwd(const float* plow, int64_t sn, int64_t sc, int64_t sh, int64_t sw,
                         const int64_t* target, const float* class_weights, int kind, float label_smoothing, float eps,
                         int N, int C, int H, int W, int rep_h, int rep_w, float* ws, float* losses, void* stream);
int ydl_seg_loss_rep_bwd(const float* plow, int64_t sn, int64_t sc, int64_t sh, int64_t sw,
                         const int64_t* target, const float* class_weights, int kind, float label_smoothing, float eps,
                         int N, int C, int H, int W, int rep_h, int rep_w, const float* ws,
                         const float* dloss /* device scalar, NULL = 1 */, float* dlow, void* stream);

/* The replicated tail in one pass each way, from the stored LOGITS x (NHWC compute dtype, rows of stride ldx, C <= 32):
 * forward = ydl_softmax_fwd at the stored resolution + ydl_seg_loss_rep_fwd without the probabilities in memory; backward =
 * ydl_seg_loss_rep_bwd + ydl_softmax_bwd without dlow in memory.  Same ws layout, same `losses`, same arithmetic per pixel
 * (the per-CTA partial sums are associated differently: several pixels per thread, fewer CTAs).
 * counts: ydl_seg_tail_count_bytes(...) bytes, 16-byte aligned: the forward leaves the per-pixel label counts there, one byte
 * per class and 16 (C <= 16) or 32 bytes per stored pixel, and the backward reads them instead of the labels.  Where
 * rep_h * rep_w > 255 a count does not fit a byte: the size is 0, counts may be NULL and the backward counts the labels again.
 * dx: rows of stride lddx in x's dtype; channels [C, round_up(C, 8)) are written as zeros where they fit into lddx, as
 * ydl_softmax_bwd writes them, and nothing beyond. */
int64_t ydl_seg_tail_count_bytes(int N, int C, int H, int W, int rep_h, int rep_w);
int ydl_seg_tail_fwd(int dtype, const void* x, int ldx, const int64_t* target, const float* class_weights /* NULL = ones */,
                     int kind, float label_smoothing, float eps, int N, int C, int H, int W, int rep_h, int rep_w,
                     float* ws, float* losses, uint8_t* counts, void* stream);
int ydl_seg_tail_bwd(int dtype, const void* x, int ldx, const uint8_t* counts, const int64_t* target,
                     const float* class_weights, float label_smoothing, int N, int C, int H, int W, int rep_h, int rep_w,
                     const float* ws, const float* dloss /* device scalar, NULL = 1 */, void* dx, int lddx, void* stream);

/* ---- optimizer: SGD(nesterov) + EMA on flat arenas --------------------------------------------------- */
/* params/grads/momentum are flat f32 arenas laid out [decay group | no-decay group]; ema spans
 * n_params + n_buffers (BN running stats follow the params in both `params` and `ema`).
 * first_step != 0: momentum buffer is initialised with the gradient (torch.optim.SGD semantics). */
int ydl_sgd_ema_step(float* params, const float* grads, float* momentum, float* ema,
                     int64_t n_decay, int64_t n_params, int64_t n_total,
                     float lr_decay_group, float lr_nodecay_group, float mom, float weight_decay, float grad_scale,
                     int first_step, float ema_decay /* <0: skip EMA */, void* stream);

/* graph-capturable form: hyper_dev = device float[7] {lr_weights, lr_bn, lr_bias, momentum, weight_decay, grad_scale,
 * ema_decay}; lr_index selects the learning rate of this run (0 weights, 1 BN weights, 2 biases) */
int ydl_sgd_ema_step_dev(float* params, const float* grads, float* momentum, float* ema,
                         int64_t n_decay, int64_t n_params, int64_t n_total, const float* hyper_dev,
                         int lr_index, int use_weight_decay, int first_step, int use_ema, void* stream);

/* every run of one step in one launch: runs_dev = device int64[nruns][6] rows {offset (elements into all four arenas), n_decay,
 * n_params, n_total, lr_index, flags: bit 0 weight decay, bit 1 first step}, each row with the meaning of the arguments of
 * ydl_sgd_ema_step_dev applied at `offset`; max_run = the largest n_total (grid sizing).  The arenas are 16-byte aligned
 * (refused otherwise: the walk reads them in 16-byte groups); the rows are read on the device unchecked: the caller keeps them
 * inside the arenas. */
int ydl_sgd_ema_step_multi(float* params, const float* grads, float* momentum, float* ema, const int64_t* runs_dev,
                           int nruns, int64_t max_run, const float* hyper_dev, int use_ema, void* stream);

/* ---- optimizer: Adam / AdamW / RMSProp + EMA on flat arenas (torch.optim.{Adam,AdamW,RMSprop}, single-tensor path) ---- */
/* rule: YDL_OPT_ADAM (coupled decay), YDL_OPT_ADAMW (decoupled decay), YDL_OPT_RMSPROP (not centered).
 * state1 / state2 are flat f32 arenas like `momentum` above, zero before the first step: Adam and AdamW keep exp_avg in
 * state1 and exp_avg_sq in state2; RMSProp keeps the momentum buffer in state1 (untouched when beta1 == 0) and square_avg
 * in state2.  Elements [0, n_decay) take the weight decay, [0, n_params) are updated, [0, n_total) feed the EMA.
 * Every factor that torch computes in Python double precision is computed by the CALLER in double and handed over rounded
 * once to f32:
 *   step_size    Adam/AdamW: lr / (1 - beta1^t);  RMSProp: lr
 *   bc2_sqrt     Adam/AdamW: sqrt(1 - beta2^t);   RMSProp: unused
 *   decay_mul    AdamW: 1 - lr * weight_decay (p *= decay_mul on the decay range);  others: unused
 *   weight_decay Adam/RMSProp: g += weight_decay * p on the decay range;  AdamW: unused
 *   beta1        Adam/AdamW: beta1;  RMSProp: momentum          one_minus_beta1 = 1 - beta1 (Adam/AdamW)
 *   beta2        Adam/AdamW: beta2;  RMSProp: alpha             one_minus_beta2 = 1 - beta2 (or 1 - alpha)
 * t is the step count of the parameters of THIS call (all of them share it).  g = grad * grad_scale. */
#define YDL_OPT_ADAM 1
#define YDL_OPT_ADAMW 2
#define YDL_OPT_RMSPROP 3
int ydl_optim_ema_step(int rule, float* params, const float* grads, float* state1, float* state2, float* ema,
                       int64_t n_decay, int64_t n_params, int64_t n_total,
                       float step_size, float bc2_sqrt, float decay_mul, float weight_decay,
                       float beta1, float beta2, float one_minus_beta1, float one_minus_beta2, float eps,
                       float grad_scale, float ema_decay /* <0: skip EMA */, void* stream);

/* graph-capturable form: hyper_dev = device float[YDL_OPT_HYPER_FLOATS]
 *   [0..2] lr of {weights, BN weights, biases}   [3] beta1 | momentum   [4] weight_decay   [5] grad_scale   [6] ema_decay
 *   [7] beta2 | alpha   [8] eps   [9] 1 - beta1   [10] 1 - beta2 | 1 - alpha   [11] decay_mul of the weights group
 *   [12 + 4c + i] step_size of bias-correction class c for lr index i (i = 0..2)   [12 + 4c + 3] bc2_sqrt of class c
 * A bias-correction class is a set of parameters with the same step count t (c < YDL_OPT_MAX_CLASSES); RMSProp has no
 * correction: it reads lr from [lr_index] and ignores bc_class. */
#define YDL_OPT_MAX_CLASSES 16
#define YDL_OPT_HYPER_FLOATS 76
int ydl_optim_ema_step_dev(int rule, float* params, const float* grads, float* state1, float* state2, float* ema,
                           int64_t n_decay, int64_t n_params, int64_t n_total, const float* hyper_dev,
                           int lr_index, int bc_class, int use_weight_decay, int use_ema, void* stream);

/* every run of one step in one launch: runs_dev = device int64[nruns][8] rows {offset (elements into all five arenas), n_decay,
 * n_params, n_total, lr_index, flags: bit 0 weight decay, bc_class, 0}, each row with the meaning of the arguments of
 * ydl_optim_ema_step_dev applied at `offset`; max_run = the largest n_total (grid sizing).  The arenas are 16-byte aligned;
 * the rows are read on the device unchecked: the caller keeps them inside the arenas. */
int ydl_optim_ema_step_multi(int rule, float* params, const float* grads, float* state1, float* state2, float* ema,
                             const int64_t* runs_dev, int nruns, int64_t max_run, const float* hyper_dev, int use_ema,
                             void* stream);

/* ---- evaluation: argmax + confusion matrix (val_diceloss.py:37-75) ---------------------------------- */
int ydl_confusion_matrix(const float* pred, int64_t sn, int64_t sc, int64_t sh, int64_t sw,
                         const int64_t* target, int N, int C, int H, int W, int ignore_index,
                         int64_t* matrix /* [C][C], accumulated */, void* stream);

/* ---- DCNv3 (models/ops_dcnv3/src/cuda/dcnv3_cuda.h:15-31) -------------------------------------------------------
 * Forward: the reference's argument order (tensors, kernel/stride/pad/dilation, group, group_channels, offset_scale),
 * followed by the sizes the reference reads off its tensors.  Backward: the same, except that grad_output sits with the
 * other tensors (the reference passes it after offset_scale, dcnv3_cuda.h:24-31) and the three gradients are caller-owned
 * outputs instead of a returned vector.  `im2col_step` has no counterpart (no batch chunking).  dtype also accepts
 * YDL_F16 here (the reference dispatches AT_DISPATCH_FLOATING_TYPES_AND_HALF, dcnv3_cuda.cu:69,147). */
int ydl_dcnv3_fwd(int dtype, const void* input, const void* offset, const void* mask, void* output,
                  int kernel_h, int kernel_w, int stride_h, int stride_w, int pad_h, int pad_w,
                  int dilation_h, int dilation_w, int group, int group_channels, float offset_scale,
                  int N, int H_in, int W_in, int H_out, int W_out, void* stream);
/* Border rule of the sampling positions (process-wide, read at launch time), the one case where the reference has two answers:
 *   0 (default)  a position exactly at -1 is inside, ">= -1": dcnv3_core_pytorch, functions/dcnv3_func.py:148-189 (F.grid_sample,
 *                padding zeros) — the form of the op the oracle and every golden vector of this repo come from;
 *   1            "> -1" as the CUDA op tests it, dcnv3_im2col_cuda.cuh:262,334,428: such a point has no value and no gradient.
 * A binding that replaces DCNv3Function's CUDA extension selects 1 once at import time. */
void ydl_dcnv3_set_border_rule(int rule);
int ydl_dcnv3_get_border_rule(void);
/* grad_input must be zeroed by the caller (f32 atomics); grad_offset/grad_mask are fully written. */
int ydl_dcnv3_bwd(int dtype, const void* input, const void* offset, const void* mask, const void* grad_output,
                  float* grad_input, float* grad_offset, float* grad_mask,
                  int kernel_h, int kernel_w, int stride_h, int stride_w, int pad_h, int pad_w,
                  int dilation_h, int dilation_w, int group, int group_channels, float offset_scale,
                  int N, int H_in, int W_in, int H_out, int W_out, void* stream);

/* ---- deformable convolution (torchvision.ops.deform_conv2d: DCNv1 with mask NULL, DCNv2 with a mask) --------------------------
 * Column form: ydl_deform_gather writes col[pix][k*C + c] = mask * bilinear(x at the deformed tap k), k = i*kw + j, pix = (n*Ho + ho)*Wo
 * + wo, in the compute dtype; with ones_column the element col[pix][kh*kw*C] is 1 (a bias as one more weight column); elements up to
 * ldc are zero.  The convolution is then a 1x1 GEMM (ydl_conv_fwd / _fwd_sums, ydl_conv_dgrad, ydl_conv_wgrad) with Cin = kh*kw*C (+1)
 * over col, whose weight [Cout][kh*kw*C] is the KRSC weight itself.  x: NHWC rows of ldx elements; offset: rows of ldo, (dy, dx)
 * interleaved per kernel point and offset group, 2*G*kh*kw values; mask: rows of ldm, G*kh*kw values, or NULL; mask_sigmoid: the
 * mask holds logits and the kernels apply the sigmoid (and its derivative).  G offset groups; channel c is in group c / (C/G).
 * Validity is tested per bilinear corner (no outer test of the sampling position: see INTEGRATION.md for the -1 border). */
int ydl_deform_gather(int dtype, const void* x, int ldx, const void* offset, int ldo, const void* mask, int ldm, int mask_sigmoid,
                      void* col, int ldc, int ones_column, int N, int H, int W, int C, int Ho, int Wo, int kh, int kw,
                      int sh, int sw, int ph, int pw, int dh, int dw, int G, void* stream);
/* Backward from dcol (rows of ldc, the gradient of col): grad_input f32 [N][H][W][C] dense, ACCUMULATED with f32 atomics (zero it
 * first; NULL = not needed); grad_offset f32 [pix][2*G*kh*kw] and grad_mask f32 [pix][G*kh*kw] (of the logits when mask_sigmoid)
 * fully written, either may be NULL.  Kernel (ydl_debug_last_kernel(4)): the LDS-window kernel at 3x3 / stride 1 / dilation 1, the
 * per-corner-atomic kernel otherwise (or with ydl_debug_set(20, 0)). */
int ydl_deform_bwd(int dtype, const void* x, int ldx, const void* offset, int ldo, const void* mask, int ldm, int mask_sigmoid,
                   const void* dcol, int ldc, float* grad_input, float* grad_offset, float* grad_mask, int N, int H, int W, int C,
                   int Ho, int Wo, int kh, int kw, int sh, int sw, int ph, int pw, int dh, int dw, int G, void* stream);

/* ---- dilated convolution in column form (stride 1, odd k, padding d*(k-1)/2: output size = input size) ---------------------------
 * The zero-offset case of the deformable gather, as two pure gathers.  ydl_dilated_cols writes, for pix = (n*H + h)*W + w and
 * tap = ky*k + kx, col[pix][tap*C + c] = x[n, h + (ky - k/2)*d, w + (kx - k/2)*d, c], or zero outside the image: a bit-exact copy in
 * the layout of ydl_deform_gather, so the KRSC weight [Cout][k*k][C] is the weight of the 1x1 GEMM over col.  With ones_col the
 * element col[pix][k*k*C] is 1; the elements from there (or from k*k*C) up to round_up(k*k*C + ones, 8) are zero; ldc must reach
 * that far.  x: rows of ldx >= C elements (a channel slice is fine).  Any other geometry (even k, d < 1) is refused.
 * ydl_dilated_cols_bwd: dx[n,h,w,c] (+)= sum over the taps whose output pixel (h - (ky - k/2)*d, w - (kx - k/2)*d) is inside the
 * image of dcol[that pixel][tap*C + c]; f32 accumulation in registers in tap order, one store per element, no atomics and no
 * workspace (bitwise reproducible); accumulate != 0 adds the sum to the previous contents of dx (rows of lddx).
 * 16-byte accesses when C % 8 == 0 and rows are 16-byte aligned, an element path otherwise. */
int ydl_dilated_cols(int dtype, const void* x, int ldx, void* col, int ldc, int ones_col,
                     int N, int H, int W, int C, int k, int d, void* stream);
int ydl_dilated_cols_bwd(int dtype, const void* dcol, int ldc, void* dx, int lddx, int accumulate,
                         int N, int H, int W, int C, int k, int d, void* stream);

/* ---- local (windowed) self-attention: AttentionConv / AttentionStem (models/common.py:1509-1627) --------------------------------
 * NHWC rows of ld* elements in the compute dtype, f32 arithmetic.  q, k: [pix][C]; v: m value tensors, V^mm at v + mm * v_stride
 * elements (m = 1 for AttentionConv).  Per sample, channel c and pixel (h, w), over the ks*ks taps t = i*ks + j that read position
 * (h + i - ks/2, w + j - ks/2) (K and V count as 0 outside the image, the tap stays in the softmax; stride 1, 'same' padding):
 *     logit_t = q[c] * (K_t[c] + r[c][t]),  P = softmax_t(logit),  out[c] = sum_t P_t * U_t[c],  U_t = sum_mm emb[mm][t] * V^mm_t[c]
 * rel_h, rel_w: f32 [C/2][ks] each, r[c][(i,j)] = rel_h[c][i] for c < C/2 and rel_w[c - C/2][j] otherwise; both NULL: r = 0.
 * emb: f32 [m][ks*ks] (ydl_attn_stem_table_fwd), NULL: weights 1 (m must be 1).  ks in {1,3,5,7}, m <= 8, m*ks*ks <= 196.
 * lse: f32 [pix][round_up(C,8)], max + log(sum) of the softmax per (pixel, channel), kept for the backward (may be NULL in
 * inference).  Rows that are not 16-byte aligned, and a last channel group of fewer than 8, move element by element: nothing
 * outside [0, C) of a row is read or written. */
int ydl_local_attn_fwd(int dtype, const void* q, int ldq, const void* k, int ldk, const void* v, int ldv, int64_t v_stride, int m,
                       const float* rel_h, const float* rel_w, const float* emb, void* out, int ldo, float* lse,
                       int N, int H, int W, int C, int ks, void* stream);
/* Backward in gather form, no atomics, bitwise reproducible.  dq, dk, dv (rows of ldd elements; dV^mm at dv + mm * dv_stride) are written, or added into
 * with accumulate != 0.  d_rel_h / d_rel_w (f32 [C/2][ks], both or neither) and the parameter sums they need are ADDED into (zero
 * them first, or keep the running sum); demb f32 [m][ks*ks] is overwritten with dE (feed it to ydl_attn_stem_table_bwd); either
 * may be NULL.  Both go through per-block partials in ws (ydl_local_attn_bwd_ws_bytes, needed when either is asked for), merged in
 * block order. */
int64_t ydl_local_attn_bwd_ws_bytes(int C, int ks, int m);
int ydl_local_attn_bwd(int dtype, const void* q, int ldq, const void* k, int ldk, const void* v, int ldv, int64_t v_stride, int m,
                       const float* rel_h, const float* rel_w, const float* emb, const void* out, int ldo, const float* lse,
                       const void* dout, int lddo, void* dq, void* dk, void* dv, int ldd, int64_t dv_stride, int accumulate, float* d_rel_h, float* d_rel_w, float* demb, float* ws,
                       int N, int H, int W, int C, int ks, void* stream);
/* AttentionStem's mixing table (models/common.py:1600-1603): emb[mm][i*ks + j] = softmax over mm of (emb_mix @ emb_a)[mm][i] +
 * (emb_mix @ emb_b)[mm][j]; emb_mix f32 [m][Cg], emb_a / emb_b f32 [Cg][ks].  The backward ADDS the three parameter gradients. */
int ydl_attn_stem_table_fwd(const float* emb_mix, const float* emb_a, const float* emb_b, float* emb, int m, int Cg, int ks,
                            void* stream);
int ydl_attn_stem_table_bwd(const float* emb_mix, const float* emb_a, const float* emb_b, const float* emb, const float* demb,
                            float* d_emb_mix, float* d_emb_a, float* d_emb_b, int m, int Cg, int ks, void* stream);

/* ---- dense multi-head self-attention: the core of TransformerLayer / C3TR (models/common.py:79-112) ----------------------------
 * NHWC rows of ld* elements in the compute dtype, f32 arithmetic on MFMA.  The tokens of sample n are its S consecutive rows
 * [n*S, (n+1)*S); head h is the channel block [h*d, (h+1)*d) of a row.  q, k, v have their own row strides (channel blocks of one
 * buffer are fine).  Per (sample, head):  P = softmax_j(scale * q_i . k_j),  out_i = sum_j P_ij v_j;  no mask, no dropout.
 * lse: f32 [N][heads][S], max + log(sum) of each softmax row, kept for the backward (may be NULL in inference).
 * S >= 1 is free; d must be a multiple of 8 with 8 <= d <= 128 (anything else is an error).  Nothing outside rows [0, N*S) and
 * channels [0, heads*d) is read or written; rows that are not 16-byte aligned move element by element. */
int ydl_mha_fwd(int dtype, const void* q, int ldq, const void* k, int ldk, const void* v, int ldv, void* out, int ldo, float* lse,
                int N, int S, int heads, int d, float scale, void* stream);
/* Backward in gather form (P recomputed from lse; one kernel per query tile writes dq, one per key tile writes dk and dv): no
 * atomics, bitwise reproducible.  dq, dk, dv (rows of ldd elements) are written, or added into with accumulate != 0.
 * ws: ydl_mha_bwd_ws_bytes(N, S, heads) bytes, receives delta = rowsum(dout * out) in f32. */
int64_t ydl_mha_bwd_ws_bytes(int N, int S, int heads);
int ydl_mha_bwd(int dtype, const void* q, int ldq, const void* k, int ldk, const void* v, int ldv, const void* out, int ldo,
                const float* lse, const void* dout, int lddo, void* dq, void* dk, void* dv, int ldd, int accumulate, float* ws,
                int N, int S, int heads, int d, float scale, void* stream);

/* ---- pieces of the DCNv3 module around the sampling op (models/ops_dcnv3/build/.../modules/dcnv3.py:50-136) ------------
 * depth-wise k x k convolution, stride 1, 'same' padding (the `dw_conv = Conv(c, c, k, g=c)` branch, :89);
 * w is the f32 master weight [C][k*k] (= nn.Conv2d(C, C, k, groups=C).weight, shape [C,1,k,k]); k in {1,3,5,7}. */
int ydl_dwconv_fwd(int dtype, const void* x, int ldx, const float* w, void* y, int ldy, int N, int H, int W, int C,
                   int k, int p, void* stream);
int ydl_dwconv_dgrad(int dtype, const void* dy, int lddy, const float* w, void* dx, int lddx, int accumulate, int N, int H, int W,
                     int C, int k, int p, void* stream);
/* dw[C][k*k] += sum over pixels; deterministic (per-block partials in ws, fixed-order merge) */
int64_t ydl_dwconv_wgrad_ws_bytes(int C, int k);
int ydl_dwconv_wgrad(int dtype, const void* x, int ldx, const void* dy, int lddy, float* dw, float* ws, int N, int H, int W, int C,
                     int k, int p, void* stream);
/* ---- strided depth-wise convolution of the Ghost blocks (models/common.py:67-70, 253-279): stride s in {1,2}, padding k/2,
 * Ho = (H + 2*(k/2) - k)/s + 1 (Wo likewise); any C; pixel strides >= C rounded up to a 16-byte chunk and multiples of a chunk, so a
 * tensor may be a channel slice of a wider buffer (channels >= C of y / dx are never written).  (H, W) is always the INPUT size.
 * ydl_dwconv2_fwd: with stats_ws != NULL the same launch writes the per-block (sum, M2) rows of the STORED output in the format of
 * ydl_bn_stats (blocks of ydl_bn_stats_block_m() output pixels, row stride round_up(C, 8), workspace of ydl_bn_stats_ws_bytes):
 * the rows equal ydl_bn_stats(y) bit for bit.  At s = 1 the output equals ydl_dwconv_fwd and the input gradient ydl_dwconv_dgrad. */
int ydl_dwconv2_fwd(int dtype, const void* x, int ldx, const float* w, void* y, int ldy, float* stats_ws, int N, int H, int W, int C,
                    int k, int s, void* stream);
/* dx[h][w] (+)= sum w[r][t] * dy[(h+p-r)/s][(w+p-t)/s] over exact quotients inside the output (gather, no atomics) */
int ydl_dwconv2_dgrad(int dtype, const void* dy, int lddy, const float* w, void* dx, int lddx, int accumulate, int N, int H, int W,
                      int C, int k, int s, void* stream);
/* dw[C][k*k] += sum over output pixels; deterministic (per-block partials in ws, fixed-order merge) */
int64_t ydl_dwconv2_wgrad_ws_bytes(int C, int k);
int ydl_dwconv2_wgrad(int dtype, const void* x, int ldx, const void* dy, int lddy, float* dw, float* ws, int N, int H, int W, int C,
                      int k, int s, void* stream);
/* ---- depth-wise transposed convolution, stride 2 (DWConvTranspose2d, models/common.py:73-76): the forms that double the map,
 * (k, p, op) in {(2,0,0), (4,1,0), (3,1,1)}: Ho = (H-1)*2 - 2p + k + op = 2H.  (H, W) is always the INPUT size; w is the f32 master
 * [C][k*k] (= nn.ConvTranspose2d(C, C, k, 2, p, op, groups=C).weight, shape [C,1,k,k]); C a multiple of 8; pixel strides as for
 * ydl_dwconv2_* (tensors may be channel slices of wider buffers).  ydl_dwtconv_supported answers on the host, without a device.
 *   fwd:   y[n,oh,ow,c] = b[c] + sum_{r,t} x[n,(oh+p-r)/2,(ow+p-t)/2,c] * w[c][r*k+t]  over exact quotients inside the input
 *   dgrad: dx[n,i,j,c] (+)= sum_{r,t} dy[n,2i-p+r,2j-p+t,c] * w[c][r*k+t]              over taps inside the output
 *   wgrad: dw[c][r*k+t] += sum_{n,i,j} x[n,i,j,c] * dy[n,2i-p+r,2j-p+t,c]; per-CTA partials in ws merged in a fixed order */
int ydl_dwtconv_supported(int C, int k, int s, int p, int op);
int ydl_dwtconv_fwd(int dtype, const void* x, int ldx, const float* w, const float* bias, void* y, int ldy, int N, int H, int W, int C,
                    int k, int p, int op, void* stream);
int ydl_dwtconv_dgrad(int dtype, const void* dy, int lddy, const float* w, void* dx, int lddx, int accumulate, int N, int H, int W,
                      int C, int k, int p, int op, void* stream);
int64_t ydl_dwtconv_wgrad_ws_bytes(int C, int k);
int ydl_dwtconv_wgrad(int dtype, const void* x, int ldx, const void* dy, int lddy, float* dw, float* ws, int N, int H, int W, int C,
                      int k, int p, int op, void* stream);
/* BN partial statistics of any NHWC tensor in the format ydl_bn_finalize consumes: nblocks = ceil(npix / block_m) rows of
 * (sum, M2) with block_m = ydl_bn_stats_block_m() */
int ydl_bn_stats_block_m(void);
int64_t ydl_bn_stats_ws_bytes(int64_t npix, int C);
int ydl_bn_stats(int dtype, const void* y, int ldy, float* ws, int64_t npix, int C, void* stream);
/* out[c] (+)= sum over pixels x[p][c]  (bias gradient of the NHWC nn.Linear layers); deterministic */
int64_t ydl_channel_sum_ws_bytes(int C);
int ydl_channel_sum(int dtype, const void* x, int ldx, float* out, float* ws, int64_t npix, int C, int accumulate, void* stream);
/* soft-max over the P = K*K sampling points of each of the G groups (modules/dcnv3.py:122-123); rows of G*P values */
int ydl_group_softmax_fwd(int dtype, const void* x, int ldx, void* y, int ldy, int64_t npix, int G, int P, void* stream);
int ydl_group_softmax_bwd(int dtype, const void* y, int ldy, const void* dy, int lddy, void* dx, int lddx, int accumulate,
                          int64_t npix, int G, int P, void* stream);
/* dst[p][0:C] (+)= (compute dtype) src[p][0:C]; src f32 (the DCNv3 op returns f32 gradients, dcnv3_cuda.cu:126-133) */
int ydl_cast_f32(int dtype, const float* src, int lds, void* dst, int ldd, int64_t npix, int C, int accumulate, void* stream);

/* ---- gradient transport helpers (yolo_dual_amd.parallel: reduce-scatter + all-gather over all peers, bf16 wire) ---------
 * dst[i] = sum over r < nchunks of src[r][i] in that fixed order (src f32 or bf16, dst f32);  dst (+)= (f32) src */
int ydl_reduce_chunks(int dtype, const void* src, float* dst, int64_t n, int nchunks, void* stream);
int ydl_cast_to_f32(int dtype, const void* src, float* dst, int64_t n, int accumulate, void* stream);

/* ---- GPU half of the per-sample input preparation -------------------------------------------------------
 * JSONSegmentDataset._resize_and_pad + the format conversion of __getitem__ (unet-lite/yolo5-seg/seg_diceloss_yolov5.py:
 * 309-349): img.resize((new_w,new_h), Image.BILINEAR) pasted on a (128,128,128) canvas, /255, HWC -> CHW float32.
 * src: uint8 [h][w][3] on the device; dst: float [3][S][S]; tmp: uint8 [h][new_w][3] scratch (may be NULL when new_w == w).
 * The arithmetic is Pillow's ImagingResample for 8-bit images (horizontal pass, 8-bit intermediate, vertical pass; 22-bit
 * fixed-point coefficients): the tables are built on the host in double exactly like Pillow's precompute_coeffs /
 * normalize_coeffs_8bpc (yolo_dual_amd/data.py) — bounds int [out][2] = (first source index, tap count), coef int
 * [out][ksize].  The kernels trust the tables (first + count <= source size).  fill = canvas grey level (128). */
int ydl_letterbox_image(const void* src, int h, int w, void* tmp, float* dst, int S, int new_w, int new_h,
                        int pad_left, int pad_top, const int* xbounds, const int* xcoef, int xksize,
                        const int* ybounds, const int* ycoef, int yksize, int fill, void* stream);
/* mask.resize((new_w,new_h), Image.NEAREST) pasted on a 0 canvas, np.clip(., 0, clip_max) (:303), int64 (:315).
 * src: uint8 [h][w]; dst: int64 [S][S]; xtab int[new_w] / ytab int[new_h]: Pillow's ImagingScaleAffine source indices
 * (sequential double additions, built on the host). */
int ydl_letterbox_mask(const void* src, int h, int w, int64_t* dst, int S, int new_w, int new_h, int pad_left,
                       int pad_top, const int* xtab, const int* ytab, int clip_max, void* stream);

/* ---- the dataset's random augmentations on the GPU (seg_diceloss_yolov5.py:75-185): uint8 in, uint8 out, same size -------------
 * Images are [h][w][3] RGB, label maps [h][w]; src and dst are distinct device buffers of h*w*channels bytes; sides below 32768.
 * Every op is byte for byte what Pillow 12 computes; the values Pillow derives once per call on the host (rotation matrix, box
 * weights, resampling tables) are arguments, built the same way in yolo_dual_amd/data.py.  Ops that leave the label map alone
 * (brightness, contrast, blur) have no label-map entry. */
/* ImageOps.mirror (horizontal != 0) / ImageOps.flip (horizontal == 0); channels 3 or 1 */
int ydl_aug_flip(const void* src, void* dst, int h, int w, int channels, int horizontal, void* stream);
/* Image.rotate(angle, BILINEAR): a0..a5 = Image.rotate's inverse affine matrix with the translation folded in (double); source
 * position a0*(x+0.5) + a1*(y+0.5) + a2, bilinear in double without FMA contraction, truncated; 0 outside the source */
int ydl_aug_rotate_image(const void* src, void* dst, int h, int w, double a0, double a1, double a2, double a3, double a4, double a5,
                         void* stream);
/* Image.rotate(angle, NEAREST): the same matrix in 16.16 fixed point, a_k = floor(v*65536 + 0.5) with a2 / a5 taken of
 * a2 + a0/2 + a1/2 (a5 + a3/2 + a4/2); source index (a2 + a1*y + a0*x) >> 16; 0 outside */
int ydl_aug_rotate_mask(const void* src, void* dst, int h, int w, int64_t a0, int64_t a1, int64_t a2, int64_t a3, int64_t a4,
                        int64_t a5, void* stream);
/* ImageEnhance.Brightness(img).enhance(factor): float(factor * px), clamped to [0, 255], truncated */
int ydl_aug_brightness(const void* src, void* dst, int h, int w, float factor, void* stream);
/* ImageEnhance.Contrast(img).enhance(factor): d = int(mean(convert("L")) + 0.5), then d + factor*(px - d) in single precision.
 * sum_ws: 16 bytes of device memory, 8-byte aligned (cleared, then the exact integer luminance sum and d, formed on the device) */
int ydl_aug_contrast(const void* src, void* dst, int h, int w, float factor, void* sum_ws, void* stream);
/* one box pass of ImageFilter.GaussianBlur (BoxBlur.c) along x (vertical == 0) or y: radius = int(fr), ww = uint32(2^24 / (2 fr + 1))
 * with the division in float, fw = (2^24 - (2 radius + 1) ww) / 2; a Gaussian blur is three x passes, then three y passes */
int ydl_aug_box_blur(const void* src, void* dst, int h, int w, int vertical, int radius, int ww, int fw, void* stream);
/* img.crop((x1, y1, x1+cw, y1+ch)).resize((w, h), BILINEAR): ydl_letterbox_image's resampler on the box, tables for cw -> w and
 * ch -> h (NULL for a side that does not change); tmp: uint8 [ch][w][3] scratch, distinct from src and dst (may be NULL when cw == w) */
int ydl_aug_crop_image(const void* src, int h, int w, int x1, int y1, int cw, int ch, void* tmp, void* dst, const int* xbounds,
                       const int* xcoef, int xksize, const int* ybounds, const int* ycoef, int yksize, void* stream);
/* mask.crop(...).resize((w, h), NEAREST): xtab int[w] / ytab int[h] index the box (ydl_letterbox_mask's tables for cw -> w, ch -> h) */
int ydl_aug_crop_mask(const void* src, int h, int w, int x1, int y1, int cw, int ch, void* dst, const int* xtab, const int* ytab,
                      void* stream);

/* ---- zero fills (the taped region issues no ATen kernel: buffers that need defined contents are cleared through these) ----
 * ydl_fill_zero: `bytes` bytes at dst (hipMemsetAsync);  ydl_zero2d: dst[p][0:C] = 0 for npix rows of pixel stride ldd */
int ydl_fill_zero(void* dst, int64_t bytes, void* stream);
int ydl_zero2d(int dtype, void* dst, int ldd, int64_t npix, int C, void* stream);

/* ---- prediction path (csrc/predict.hip): label maps, their metrics and pictures ----------------------------------------------
 * What the reference does with a trained model besides mIoU: unet-lite/Resnet50/test.py:410-464 (SegmentationMetrics),
 * yolo5-seg/val_diceloss.py:103-119 (overlay), seg_diceloss_yolov5.py:810-830 (mask_to_rgb, visualize_prediction_difference) and
 * :753-771 (seg_labels_to_class_weights).  Label maps are uint8 with an image stride and a row stride in bytes.  Every entry point
 * checks its arguments on the host and launches nothing when it refuses them.
 *
 * ydl_argmax_labels: labels[n][h*rep_h + i][w*rep_w + j] = argmax_c x[n*sn + c*sc + h*sh + w*sw] for i < rep_h, j < rep_w (the lazy
 * nearest replication of the tape folded into the store).  x: f32 or bf16 scores with four ELEMENT strides: the tape's NHWC rows
 * (sc = 1, sw = ld) or an NCHW tensor.  torch.argmax's rule: the first maximum wins, a NaN counts as the maximum and the first NaN
 * wins.  1 <= C <= 32.  With sc == 1, 16-byte aligned rows and sw >= C rounded up to a 16-byte chunk a thread reads its pixel as
 * 16-byte vectors, otherwise element by element.  Nothing outside the N * (H*rep_h) rows of W*rep_w bytes is written. */
int ydl_argmax_labels(int dtype, const void* x, int64_t sn, int64_t sc, int64_t sh, int64_t sw, int N, int C, int H, int W,
                      int rep_h, int rep_w, uint8_t* labels, int64_t ldl_n, int64_t ldl_h, void* stream);
/* labels[n][ho][wo] = argmax_c bilinear_resize(softmax_c(x))[n][c][ho][wo], align_corners = False, (Hi, Wi) -> (Ho, Wo): the exit of
 * a model whose last Softmax is followed by the resize to its output size, without writing the probabilities or their resized copy.
 * x: NHWC rows of ldx elements, f32 or bf16.  The f32 arithmetic is ydl_softmax_fwd's followed by ydl_resize_fwd's (mode 1),
 * expression for expression: the labels are the argmax of the very values those two launches would have produced. */
int ydl_softmax_resize_labels(int dtype, const void* x, int ldx, int N, int C, int Hi, int Wi, int Ho, int Wo,
                              uint8_t* labels, int64_t ldl_n, int64_t ldl_h, void* stream);
/* dst[n][i][j] = src[n][y0 + si][x0 + sj]: the crop box (y0, x0, hc, wc) of every image resized to Ho x Wo by ATen's nearest rule,
 * si = min((int)floorf(i * ((float)hc / Ho)), hc - 1) in f32, sj likewise (F.interpolate(mode='nearest') of the box).  With the box
 * = letterbox_geometry's interior and (Ho, Wo) = the source image's size this undoes the letterbox.  (test.py:419-424 is NOT this:
 * its unsqueeze(0) makes the call a 1-D resize along the width, and it raises for int64 predictions.) */
int ydl_labels_resize(const uint8_t* src, int64_t lds_n, int64_t lds_h, int N, int y0, int x0, int hc, int wc,
                      uint8_t* dst, int64_t ldd_n, int64_t ldd_h, int Ho, int Wo, void* stream);
/* matrix[t][p] += 1 over the pixels of two label maps (int64 [C][C], rows = target).  target: uint8, or int64 with
 * target_is_i64 != 0, strides in elements.  A pixel is dropped when t < 0, t >= C, t == ignore_index or p >= C
 * (val_diceloss.py:50-58, test.py:431); ignore_index = -1 ignores nothing.  1 <= C <= 32. */
int ydl_confusion_labels(const uint8_t* pred, int64_t ldp_n, int64_t ldp_h, const void* target, int target_is_i64,
                         int64_t ldt_n, int64_t ldt_h, int N, int H, int W, int C, int ignore_index, int64_t* matrix, void* stream);
/* counts[v] += 1 for each of the n labels (uint8, or int64 with is_i64 != 0); counts holds nbins + 1 int64, the last entry collects
 * the labels outside [0, nbins).  1 <= nbins <= 4096. */
int ydl_label_bincount(const void* labels, int is_i64, int64_t n, int nbins, int64_t* counts, void* stream);
/* out: uint8 [N][H][W][3]; pred / target: dense uint8 [N][H][W]; palette: uint8 [npal][3], npal <= 256.
 *   mode 0, colour (mask_to_rgb):  palette[pred], (0,0,0) where pred >= npal
 *   mode 1, difference (visualize_prediction_difference):  (255,0,255) where pred != target, else as mode 0
 *   mode 2, overlay (val_diceloss.py:103-119): base = uint8(img * 255) by truncation (img: f32 [N][3][H][W], the product in f32,
 *           values outside [0, 255] saturate); out = rint(0.5 * base + 0.5 * colour), half to even.  With bgr != 0 the base's
 *           channels are swapped and the palette triple is written unswapped, as the reference does.  The rounding is OpenCV's
 *           documented saturate_cast<uchar>(float); it has not been pinned against a cv2 build. */
int ydl_labels_render(int mode, const uint8_t* pred, const uint8_t* target, const float* img, const uint8_t* palette, int npal,
                      uint8_t* out, int N, int H, int W, int bgr, void* stream);

/* ---- ConvNeXt block pieces (csrc/convnext.hip) -----------------------------------------------------------------------------
 * NHWC rows with element strides (any tensor may be a channel slice of a wider buffer: channels outside [0, C) are neither read
 * into a result nor written), f32 or bf16 storage, f32 arithmetic, 16-byte accesses (data pointers 16-byte aligned, strides whole
 * chunks, C a multiple of 8).  No atomics: every per-channel sum goes through one partial row per CTA in `ws` (the *_ws_bytes
 * functions size it; pure host functions) and a fixed-order fold in double, so two runs give the same bits.  Parameter gradients
 * are ADDED into their destination, which holds zeros or a running sum.  Bad arguments are refused on the host before any launch.
 *
 * LayerNorm over C at every pixel, 8 <= C <= 1024 (ydl_ln_supported):
 *   u = x + pre_bias[c] (pre_bias: f32 [C], or NULL), mu = mean_c u, var = mean_c (u - mu)^2 (second pass over the
 *   registers), r = 1 / sqrtf(var + eps), y = (u - mu) * r * gamma[c] + beta[c]; stats: f32 [npix][2] = (mu, r), or NULL (eval).
     The f32 parameter rows need no alignment.
 * Backward, one pass over x and dy, with g = dy * gamma and xh = (u - mu) * r:
 *   dx (+)= r * (g - mean_c g - xh * mean_c (g * xh)) (accumulate != 0 adds in f32 with one rounding),
 *   dgamma[c] += sum_p dy * xh, dbeta[c] += sum_p dy, dpre_bias[c] += sum_p (the new dx term); dpre_bias may be NULL. */
int ydl_ln_supported(int C);
int ydl_ln_fwd(int dtype, const void* x, int ldx, const float* pre_bias, const float* gamma, const float* beta, float eps,
               void* y, int ldy, float* stats, int64_t npix, int C, void* stream);
int64_t ydl_ln_bwd_ws_bytes(int64_t npix, int C);
int ydl_ln_bwd(int dtype, const void* x, int ldx, const float* pre_bias, const float* gamma, const float* stats,
               const void* dy, int lddy, void* dx, int lddx, int accumulate, float* dgamma, float* dbeta, float* dpre_bias,
               float* ws, int64_t npix, int C, void* stream);
/* bias + exact GELU: u = z + bias[c], y = 0.5 * u * (1 + erff(u / sqrt 2)).  Backward: dz = dy * (Phi(u) + u * phi(u)),
 * dbias[c] += sum_p dz; dz may be dy's own buffer. */
int ydl_bias_gelu_fwd(int dtype, const void* z, int ldz, const float* bias, void* y, int ldy, int64_t npix, int C, void* stream);
int64_t ydl_bias_gelu_bwd_ws_bytes(int64_t npix, int C);
int ydl_bias_gelu_bwd(int dtype, const void* z, int ldz, const float* bias, const void* dy, int lddy, void* dz, int lddz,
                      float* dbias, float* ws, int64_t npix, int C, void* stream);
/* layer-scaled residual with per-sample keep factors (stochastic depth, "row" mode): out[n][p][c] = x + keep[n] * gamma[c] * y over
 * N samples of hw pixels; keep: f32 [N], or NULL meaning 1.  The product is formed in f32 and added to x with one rounding; a
 * sample with keep[n] == 0 gets x bit for bit.  Backward: dy = keep[n] * gamma[c] * dout, dgamma[c] += sum keep[n] * dout * y,
 * dx (+)= dout; dx may be NULL (the caller aliases the residual's gradient). */
int ydl_scale_res_fwd(int dtype, const void* y, int ldy, const float* gamma, const float* keep, const void* x, int ldx,
                      void* out, int ldo, int N, int64_t hw, int C, void* stream);
int64_t ydl_scale_res_bwd_ws_bytes(int N, int64_t hw, int C);
int ydl_scale_res_bwd(int dtype, const void* dout, int lddo, const void* y, int ldy, const float* gamma, const float* keep,
                      void* dy, int lddy, void* dx, int lddx, int accumulate, float* dgamma, float* ws, int N, int64_t hw,
                      int C, void* stream);

/* ---- squeeze-and-excitation gate (csrc/se.hip) ------------------------------------------------------------------------------
 * SqueezeExcitation(C, Cs) per sample n:  p[c] = mean_hw x[n, :, c],  h = W1 p + b1,  a = act(h),  z = W2 a + b2,  g = scale(z),
 * out = x * g[n, c].  x is NHWC with an element stride (it may be a channel slice of a wider buffer), f32 or bf16, 16-byte aligned,
 * C a multiple of 8 in 8..2048, Cs in 1..512 (ydl_se_supported).  W1 [Cs][C], b1 [Cs], W2 [C][Cs], b2 [C] are the f32 masters as they
 * stand: they are read by element and need no alignment.  act: YDL_ACT_RELU or YDL_ACT_SILU; the gate code selects scale.  f32
 * arithmetic, no atomics, fixed summation order: two runs give the same bits.  Bad arguments are refused on the host before any launch.
 *
 * ydl_se_pool_fwd: ws[n][s][c] = the sum over slice s of sample n's pixels of x (y == NULL) or of x * y (the gate gradient
 *   dgate = sum_hw dy * x); S = ydl_se_pool_splits(N, HW) slices of ceil(HW / S) pixels, ws of ydl_se_pool_ws_bytes (host functions).
 * ydl_se_excite_fwd, one launch: folds the S partial rows in order, pooled = sum / HW, then h, z and gate; all four are written
 *   (pooled, z, gate: f32 [N][C]; h: f32 [N][Cs]) -- the backward differentiates scale at the stored z and act at the stored h.
 * ydl_se_excite_bwd, two launches: dgate is [N][S][C] partial rows (S = 1: the plain [N][C] gradient), folded in order;
 *   dz = dgate * scale'(z) (sigmoid: e / (1 + e)^2 with e = exp(-|z|); hardsigmoid: 1/6 for -3 < z < 3, else 0),
 *   dh = (W2^T dz) * act'(h), dpooled = W1^T dh [N][C]; then dW1[j][c] += sum_n dh[n][j] pooled[n][c], db1 += sum_n dh,
 *   dW2[c][j] += sum_n dz[n][c] act(h[n][j]), db2 += sum_n dz, the samples in order.  A NULL gradient pointer is skipped (a frozen
 *   parameter).  ws: ydl_se_excite_bwd_ws_bytes, holds dz [N][C] and dh [N][Cs].
 * ydl_se_scale_bwd: dx (+)= dy * gate[n][c] + dpooled[n][c] / HW in one pass; accumulate != 0 adds in f32 with one rounding. */
enum { YDL_SE_GATE_SIGMOID = 0, YDL_SE_GATE_HSIGMOID = 1 /* relu6(z + 3) / 6 */ };
int ydl_se_supported(int C, int Cs);
int ydl_se_pool_splits(int N, int64_t HW);
int64_t ydl_se_pool_ws_bytes(int N, int64_t HW, int C);
int ydl_se_pool_fwd(int dtype, const void* x, int ldx, const void* y, int ldy, float* ws, int N, int64_t HW, int C, void* stream);
int ydl_se_excite_fwd(const float* part, int S, const float* w1, const float* b1, const float* w2, const float* b2, int act,
                      int gate_kind, float* pooled, float* h, float* z, float* gate, int N, int64_t HW, int C, int Cs, void* stream);
int64_t ydl_se_excite_bwd_ws_bytes(int N, int C, int Cs);
int ydl_se_excite_bwd(const float* dgate, int S, const float* pooled, const float* h, const float* z, const float* w1,
                      const float* w2, int act, int gate_kind, float* dpooled, float* dw1, float* db1, float* dw2, float* db2,
                      float* ws, int N, int C, int Cs, void* stream);
int ydl_se_scale_bwd(int dtype, const void* dy, int lddy, const float* gate, const float* dpooled, void* dx, int lddx,
                     int accumulate, int N, int64_t HW, int C, void* stream);

/* ---- activations with a run-time parameter ----------------------------------------------------------------------------
 * The six streaming BatchNorm entry points above, each with one more argument after `act`: act_param, the parameter of the
 * activation (the negative slope of YDL_ACT_LEAKY; ignored by every other code).  The entry points without it are these with
 * act_param = 0, and refuse YDL_ACT_LEAKY.  YDL_ACT_LEAKY, YDL_ACT_HSWISH and YDL_ACT_MISH recompute z = y*scale + shift in
 * the backward, as YDL_ACT_SILU does: they need no saved output, and their backward refuses YDL_RES_BEFORE_ACT. */
int ydl_bn_act_fwd_p(int dtype, const void* y, int ldy, const float* scale, const float* shift,
                     const void* res, int ldr, int res_mode, int act, float act_param, void* out, int ldo,
                     int64_t npix, int Cp, void* stream);
int ydl_bn_act_bwd_p(int dtype, const void* y, int ldy, const void* dout, int lddo, const void* out, int ldo,
                     const float* gamma, const float* mean, const float* invstd, const float* scale, const float* shift,
                     int res_mode, int act, float act_param, void* dy, int lddy, void* dres, int lddr,
                     float* dgamma, float* dbeta, int accumulate_param_grads,
                     float* ws, int64_t npix, int C, int Cp, void* stream);
int ydl_bn_act_fwd_sums_p(int dtype, const void* y, int ldy, const float* sums, int sums_ld, int64_t count,
                          const float* gamma, const float* beta, float eps, float momentum,
                          float* running_mean, float* running_var, float* mean, float* invstd, float* scale, float* shift,
                          int replication, const void* res, int ldr, int res_mode, int act, float act_param, void* out, int ldo,
                          int64_t npix, int C, int Cp, void* stream);
int ydl_bn_act_bwd_sums_p(int dtype, const void* y, int ldy, const void* dout, int lddo, const void* out, int ldo,
                          const float* mean, const float* invstd, const float* scale, const float* shift,
                          int res_mode, int act, float act_param, void* dy, int lddy, void* dres, int lddr,
                          float* dgamma, float* dbeta, int accumulate_param_grads,
                          float* sums, int64_t npix, int C, int Cp, void* stream);
int ydl_bn_act_bwd_apply_sums_p(int dtype, const void* y, int ldy, const void* dout, int lddo, const void* out, int ldo,
                                const float* mean, const float* invstd, const float* scale, const float* shift,
                                int res_mode, int act, float act_param, void* dy, int lddy, void* dres, int lddr,
                                float* dgamma, float* dbeta, int accumulate_param_grads,
                                float* sums, int64_t npix, int C, int Cp, void* stream);
int ydl_bn_act_bwd_reduce_sums_p(int dtype, const void* y, int ldy, const void* dout, int lddo, const void* out, int ldo,
                                 const float* mean, const float* invstd, const float* scale, const float* shift,
                                 int res_mode, int act, float act_param, void* dres, int lddr, float* sums, int64_t npix, int C, int Cp,
                                 void* stream);

/* ---- learnable Conv activations (csrc/act.hip) --------------------------------------------------------------------------
 * AconC (utils/activations.py): out = d * sigmoid(beta * d) + p2 * z with d = (p1 - p2) * z, per channel, on the materialised
 * BatchNorm output z.  NHWC with pixel strides, 16-byte accesses (pointers 16-byte aligned, strides whole chunks); p1 / p2 hold C
 * floats and channels [C, Cp) are computed with zeros.  beta is read at beta[sample * beta_stride + c], a sample being hw
 * consecutive pixels: beta_stride = 0 is AconC's single row, a per-sample row is what a generated beta (MetaAconC) needs. */
int ydl_acon_fwd(int dtype, const void* z, int ldz, const float* p1, const float* p2, const float* beta, int64_t beta_stride,
                 void* out, int ldo, int64_t npix, int64_t hw, int C, int Cp, void* stream);
int64_t ydl_acon_bwd_ws_bytes(int64_t npix, int64_t hw, int64_t beta_stride, int Cp);
/* one pass over z and dout: dz (dz_accumulate != 0: added to what dz holds, in f32 with one rounding) and the per-channel sums
 * dp1, dp2 [C] and dbeta (one row of C floats per beta row, same stride), stored or, with accumulate_param_grads != 0, added.
 * One partial row per CTA in ws and a fixed-order fold: no atomics, two runs give the same bits. */
int ydl_acon_bwd(int dtype, const void* z, int ldz, const void* dout, int lddo, const float* p1, const float* p2, const float* beta,
                 int64_t beta_stride, void* dz, int lddz, int dz_accumulate, float* dp1, float* dp2, float* dbeta,
                 int accumulate_param_grads, float* ws, int64_t npix, int64_t hw, int C, int Cp, void* stream);
/* FReLU's merge: out = max(a, b).  The backward routes dout to the larger operand and gives half to each on a tie (torch.max(a, b));
 * da or db may be NULL (not wanted); *_accumulate != 0 adds to what the gradient holds, in f32 with one rounding. */
int ydl_max2_fwd(int dtype, const void* a, int lda, const void* b, int ldb, void* out, int ldo, int64_t npix, int Cp, void* stream);
int ydl_max2_bwd(int dtype, const void* a, int lda, const void* b, int ldb, const void* dout, int lddo, void* da, int ldda,
                 int da_accumulate, void* db, int lddb, int db_accumulate, int64_t npix, int Cp, void* stream);

/* ---- launch-list replay: the training step without its host wall -------------------------------------------------------
 * The reference's hot loop (seg_diceloss_yolov5.py:1084-1103) issues the same sequence of device work every step.  The host
 * side records ONE step — every entry-point call above with its arguments, the stream it went to, and the cross-stream
 * event edges — into a ydl_replay and re-issues it with one call per step: no Python, no ctypes marshalling per launch, the
 * same kernels on the same streams with the same dependencies as the eager step (so the eager step's overlap survives).
 * Preconditions (the caller's job, yolo_dual_amd/replay.py): every buffer a recorded call names must stay valid and at the same
 * address for the life of the ydl_replay (a private allocator pool), and every device operation of the step must be in the
 * list.  Streams are named by slot: the table passed to ydl_replay_run maps slot -> hipStream_t. */
typedef struct ydl_replay ydl_replay;
ydl_replay* ydl_replay_create(void);
void ydl_replay_destroy(ydl_replay* r);
/* number / names of the recordable entry points (index = `fn` below); generated from this header (tools/gen_replay.py) */
int ydl_replay_fn_count(void);
const char* ydl_replay_fn_name(int fn);
/* append one call: args = the entry point's parameters before `stream`, one 8-byte slot each (integers and pointers as
 * int64, floats as the bits of a double; a ydl_conv_geom* / ydl_bnred* slot holds a HOST pointer whose struct is copied) */
int ydl_replay_add_call(ydl_replay* r, int fn, const int64_t* args, int nargs, int stream_slot);
/* cross-stream edge: hipEventRecord(event[id], stream[slot]) / hipStreamWaitEvent(stream[slot], event[id]) */
int ydl_replay_add_event_record(ydl_replay* r, int event_id, int stream_slot);
int ydl_replay_add_event_wait(ydl_replay* r, int event_id, int stream_slot);
int ydl_replay_size(const ydl_replay* r);
/* re-issue operations [first, last) in order; h_streams: host array of nstreams hipStream_t.  Stops at the first failing call
 * (its status is returned, ydl_last_error() says which operation). */
int ydl_replay_run(ydl_replay* r, int first, int last, void* const* h_streams, int nstreams);

#ifdef __cplusplus
}
#endif
#endif /* YDL_H_ */
