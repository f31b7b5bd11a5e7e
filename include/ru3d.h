/*
 * ru3d.h - C ABI of the MI355X-native 3D U-Net training hot path (libru3d.so).
 *
 * The reference (icrdr/3D-UNet-Renal-Anatomy-Extraction) has no FFI of its own: its hot path is
 * entered through `nn.Module.__call__` and every arithmetic op is delegated to torch.nn.  This
 * header is the boundary the build introduces *beneath* the reference's Python classes
 * (network.py / loss.py / trainer.py keep their names and signatures); each entry point cites the
 * reference call site whose arithmetic it replaces.
 *
 * Conventions
 *  - plain C only: scalars, raw device pointers, explicit shapes; no C++/torch types.
 *  - the CALLER owns every buffer, including workspaces (sizes from the *_workspace_bytes calls);
 *    the library never allocates or frees device memory and keeps no mutable global state.
 *  - activations are NDHWC ("channels last") in HBM: element (n,d,h,w,c) of a tensor lives at
 *    ptr[(((n*D+d)*H+h)*W+w)*ld + c]; `ld` (>= c) is the voxel pitch in elements, so a tensor can be
 *    a channel slice of a wider buffer (this is how the skip-concat is written in place).
 *  - every call only enqueues work on `stream` (a hipStream_t passed as void*; NULL = default
 *    stream).  No call synchronises the device.
 *  - return value: 0 = OK; < 0 = invalid argument / unsupported shape (see ru3d_last_error());
 *    > 0 = hipError_t from the launch.  Never throws, never exits.
 *  - thread safety: re-entrant; the error string is thread-local (PyTorch runs backward on its own
 *    autograd thread).
 */
#ifndef RU3D_H
#define RU3D_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RU3D_VERSION 201

/* storage dtypes of activations / packed weights (accumulation is always fp32).  RU3D_F16 is the reference's
 * mixed-precision arithmetic (apex O1: fp16 convolutions with fp32 accumulation, trainer.py:492-493, 538-542) and
 * needs loss scaling on the host side; RU3D_BF16 needs none.  A call uses ONE 16-bit type throughout. */
enum { RU3D_F32 = 0, RU3D_BF16 = 1, RU3D_F16 = 2 };

/* label dtypes accepted by the loss kernels (reference passes int64: loss.py:27) */
enum { RU3D_LABEL_I64 = 0, RU3D_LABEL_U8 = 1 };

/* which reference weight tensor a packed weight is made from, and for which kernel */
enum {
    RU3D_ROLE_CONV_FWD = 0,    /* nn.Conv3d weight [Cout][Cin][k^3]          -> forward          */
    RU3D_ROLE_CONV_DGRAD = 1,  /* nn.Conv3d weight                            -> input gradient   */
    RU3D_ROLE_CONVT_FWD = 2,   /* nn.ConvTranspose3d weight [Cin][Cout][k^3]  -> forward          */
    RU3D_ROLE_CONVT_DGRAD = 3, /* nn.ConvTranspose3d weight                   -> input gradient   */
    RU3D_ROLE_BIAS = 4         /* bias vector [Cout] -> fp32 [Cout padded] (ru3d_pack_weights only)  */
};

/* loss kinds: which reference module the finalize step reproduces */
enum {
    RU3D_LOSS_HYBIRD = 0,   /* loss.py:196-254 HybirdLoss                    */
    RU3D_LOSS_DICELOSS = 1, /* loss.py:123-166 DiceLoss                      */
    RU3D_LOSS_FOCAL = 2,    /* loss.py:169-193 FocalLoss (+ focal_loss :51)  */
    RU3D_LOSS_DICE = 3      /* loss.py:85-120  Dice (metric)                 */
};

typedef struct ru3d_tensor {
    void* ptr;          /* device pointer to element (0,0,0,0,0)        */
    int32_t n, d, h, w; /* batch and spatial extents                     */
    int32_t c;          /* channels                                      */
    int32_t ld;         /* voxel pitch in elements (>= c; split: >= cseg) */
    /* Split ("planar") channel layout, cseg != 0: the channels are c / cseg segments of cseg channels, segment s a dense
     * NDHWC tensor of its own at ptr + s * seg_stride elements (voxel pitch ld): element (n,d,h,w,ch) sits at
     * ptr[(ch / cseg) * seg_stride + (((n*D+d)*H+h)*W+w) * ld + ch % cseg].  This is how torch.cat((up, skip), dim=1)
     * (reference network.py:350) is held on the full-resolution level, where the two 32-channel halves interleaved in
     * one 128-byte row would cost every reader / writer of ONE half double line traffic: both halves stay contiguous
     * tensors and only the kernels that consume the concat (ru3d_planar_concat_supported lists them) take the pair.
     * Every other entry point rejects a split tensor. */
    int32_t cseg;
    int64_t seg_stride;
} ru3d_tensor;

int ru3d_version(void);
/* thread-local, valid until the next failing call on this thread */
const char* ru3d_last_error(void);
/* Launch log (tests): between _begin and _end the library records, on the calling thread, the name of every kernel
 * launch it checks - for the conv family the name carries the template arguments of the instantiation, e.g.
 * "conv_gather_mfma<2,6>".  _begin clears and arms the log; _end disarms it and returns the names joined by ';'
 * (thread-local, valid until the next _begin on this thread; "" if the log was never armed).  Host side only. */
void ru3d_launch_log_begin(void);
const char* ru3d_launch_log_end(void);

/* ------------------------------------------------------------------ weights ----------------- */
/* Number of bytes of the packed form of a weight (layout is private to the library and depends on
 * (cin, cout, k, stride, dtype, role); `stride` is the nn.Module's stride, 2 for the ConvTranspose3d roles). */
size_t ru3d_packed_weight_bytes(int cout, int cin, int k, int stride, int role, int dtype);
/* src: fp32 weight in the reference's layout (state_dict tensor, contiguous).  dst: packed. */
int ru3d_pack_weight(const float* src, void* dst, int cout, int cin, int k, int stride, int role, int dtype,
                     void* stream);

/* Same, for up to RU3D_PACK_MAX weights in ONE launch (a ResBlock's three convs x {forward, dgrad} + biases).
 * Channel padding: widths that are not multiples of 32 (the reference's default num_features = 30,
 * network.py:107, gives 30/60/120/240/480) run on the MFMA kernels with activations padded to the next multiple
 * of 32 and exact zeros in the pad lanes.  cout_seg / cin_seg != 0 ask for the packed weight of such a layer:
 * that dimension of the module's weight consists of (dim / seg) segments of `seg` real channels, each padded with
 * zero rows / columns to the next multiple of 32 (cin_seg = 30 for cin = 60 is the decoder's concat input
 * 30 | 30 -> 32 | 32, network.py:350).  dst is then ru3d_packed_weight_bytes(padded cout, padded cin, ...) long.
 * Role RU3D_ROLE_BIAS pads a bias vector the same way (src fp32 [cout], dst fp32 [padded cout]; k = 1). */
#define RU3D_PACK_MAX 40
typedef struct ru3d_pack_item {
    const float* src; /* fp32 weight, reference layout                  */
    void* dst;        /* packed output, ru3d_packed_weight_bytes() long  */
    int32_t cout, cin, k, stride, role;
    int32_t cout_seg, cin_seg; /* 0 = no padding of that dimension       */
} ru3d_pack_item;
int ru3d_pack_weights(const ru3d_pack_item* items, int count, int dtype, void* stream);

/* Inverse of the channel padding for a weight gradient: src = fp32 [cout_p][cin_p][taps] as the wgrad entry points
 * write it for padded activations, dst = fp32 [cout][cin][taps] (the parameter's shape), segments as above. */
int ru3d_unpad_weight_grad(const float* src, float* dst, int cout, int cin, int taps, int cout_seg, int cin_seg,
                           void* stream);

/* ------------------------------------------------------------------ convolutions ------------ */
/* nn.Conv3d(k in {1,3}, stride in {1,2}, padding=k/2) forward (network.py:394-395,403,541-547).
 * y = conv(x) + bias (+ res).  bias (fp32 [Cout]) and res may be NULL.  y_dtype may be RU3D_F32
 * while x is bf16 (the logits head). */
/* Optional scratch of ru3d_conv3d_fwd / ru3d_conv3d_dgrad (call with (dy, dx) for the latter): split-K partials of the
 * deepest level; 0 for most shapes.  ws may be NULL (the launch then takes a path that needs none). */
size_t ru3d_conv3d_workspace_bytes(const ru3d_tensor* x, const ru3d_tensor* y, int k, int stride, int dtype);
int ru3d_conv3d_fwd(const ru3d_tensor* x, const void* w_packed, const float* bias, const ru3d_tensor* res,
                    const ru3d_tensor* y, int k, int stride, int dtype, int y_dtype, void* ws,
                    size_t ws_bytes, void* stream);
/* Which kernels the conv that gathers from x and writes y (dense tensors of one dtype, no residual; transposed: the
 * fractionally strided form of ConvTranspose3d forward and the stride-2 input gradient) runs on: the launch-log names in
 * the order of preference, joined by '|', written to buf (cap bytes).  A launch runs the first whose launch-time
 * conditions (operand alignment, scratch) hold.  "stem" / "head": the small-channel kernels; "generic": no MFMA kernel
 * takes the shape.  Pure host code: no pointer is dereferenced.  < 0: bad argument or no kernel. */
int ru3d_conv3d_plan_names(const ru3d_tensor* x, const ru3d_tensor* y, int k, int stride, int transposed, int dtype,
                           char* buf, size_t cap);
/* The same forward conv FOLLOWED by the InstanceNorm statistics of its output (ResBlock: conv -> dropout ->
 * norm, network.py:411-414): y = conv(x) + bias, then mean / scale exactly as ru3d_instnorm_stats(y, ...)
 * would produce.  On the producer/consumer MFMA kernel the sums are accumulated in the conv epilogue (no
 * second pass over y); other shapes run the two kernels back to back.  Workspace from the _bytes query. */
size_t ru3d_conv3d_fwd_in_workspace_bytes(const ru3d_tensor* x, const ru3d_tensor* y, int k, int stride, int dtype);
int ru3d_conv3d_fwd_in(const ru3d_tensor* x, const void* w_packed, const float* bias, const ru3d_tensor* y, int k,
                       int stride, int dtype, const float* drop_scale, float* mean, float* scale, void* ws,
                       size_t ws_bytes, float eps, void* stream);
/* conv + InstanceNorm statistics + apply + LeakyReLU behind one entry point - a ResBlock's conv -> dropout -> norm ->
 * nonlin chain (reference network.py:405-416) and, with `res`, its tail lrelu(IN(conv2(x)) + skip):
 *     y = conv(x) + bias;  (mean, scale) as ru3d_conv3d_fwd_in;  out = lrelu((y - mean) * scale (+ res))
 * y is kept (the backward reads it).  On small levels (<= 4096 voxels per sample, 16-bit storage) the statistics, their
 * finalize and the apply are one whole-instance kernel that also sums the conv's split-K slices; elsewhere the call is
 * ru3d_conv3d_fwd_in + ru3d_in_lrelu_fwd.  Workspace: ru3d_conv3d_fwd_in_lrelu_workspace_bytes. */
size_t ru3d_conv3d_fwd_in_lrelu_workspace_bytes(const ru3d_tensor* x, const ru3d_tensor* y, int k, int stride, int dtype);
int ru3d_conv3d_fwd_in_lrelu(const ru3d_tensor* x, const void* w_packed, const float* bias, const ru3d_tensor* y, int k,
                             int stride, int dtype, const float* drop_scale, float* mean, float* scale,
                             const ru3d_tensor* res, const ru3d_tensor* out, float slope, void* ws, size_t ws_bytes,
                             float eps, void* stream);
/* 1 when a decoder ResBlock whose input is the concat of two `cseg`-channel tensors on an n x d x h x w grid can take that
 * input as a split tensor through every kernel of its forward and backward: ru3d_conv3d_fwd / _fwd_in / _fwd_in_lrelu (x),
 * ru3d_skip1x1_in_lrelu_fwd (x), ru3d_conv3d_wgrad k = 3 and k = 1 (x), ru3d_conv3d_s1_dgrad_pair (dx).  cout: the
 * block's output channels. */
int ru3d_planar_concat_supported(int n, int d, int h, int w, int cseg, int cout, int dtype);
/* input gradient of the same conv: dx = conv_dgrad(dy) (+ res).  w_packed made with ROLE_CONV_DGRAD. */
int ru3d_conv3d_dgrad(const ru3d_tensor* dy, const void* w_packed, const ru3d_tensor* res,
                      const ru3d_tensor* dx, int k, int stride, int dtype, void* ws, size_t ws_bytes,
                      void* stream);
/* The input gradient of a decoder ResBlock's two stride-1 convs of the same input in ONE launch (network.py:394 conv1
 * k3 s1 and :403 skip_conv k1 s1, :406-411): dx = conv3_dgrad(dy; w3_packed) + conv1_dgrad(dy2; w1_packed), dy and dy2
 * on the same grid with the same channel count.  `_supported` as above. */
int ru3d_conv3d_s1_dgrad_pair_supported(const ru3d_tensor* dy, const ru3d_tensor* dy2, const ru3d_tensor* dx, int dtype);
int ru3d_conv3d_s1_dgrad_pair(const ru3d_tensor* dy, const void* w3_packed, const ru3d_tensor* dy2, const void* w1_packed,
                              const ru3d_tensor* dx, int dtype, void* stream);
/* The forward of a pooling ResBlock's two stride-2 convs of the same input in ONE launch (network.py:394 conv1 k3 s2 p1,
 * :403 skip_conv k1 s2; :406-411), plus the InstanceNorm statistics of conv1's output as ru3d_conv3d_fwd_in takes them:
 *     y3 = conv3(x; w3, b3), (mean, scale) = IN statistics of Dropout3d(y3), y1 = conv1(x; w1, b1)
 * `_supported`: a fused kernel exists for the shapes; workspace: ru3d_conv3d_s2_pair_fwd_in_workspace_bytes. */
int ru3d_conv3d_s2_pair_fwd_in_supported(const ru3d_tensor* x, const ru3d_tensor* y3, const ru3d_tensor* y1, int dtype);
size_t ru3d_conv3d_s2_pair_fwd_in_workspace_bytes(const ru3d_tensor* x, const ru3d_tensor* y3, int dtype);
int ru3d_conv3d_s2_pair_fwd_in(const ru3d_tensor* x, const void* w3_packed, const float* b3, const ru3d_tensor* y3,
                               const void* w1_packed, const float* b1, const ru3d_tensor* y1, const float* drop_scale,
                               float* mean, float* scale, void* ws, size_t ws_bytes, float eps, int dtype, void* stream);
/* The input gradient of a pooling ResBlock's two stride-2 convs in ONE launch (reference network.py:394 conv1 k3 s2 p1
 * and :403 skip_conv k1 s2, both applied to the block's input, :406-411):
 *     dx = conv3_dgrad(dy; w3_packed) + conv1_dgrad(dy2; w1_packed) (+ res)
 * dy and dy2 live on the same (pooled) grid with the same channel count.  `_supported` says whether a fused kernel
 * exists for the shapes (the caller otherwise chains two ru3d_conv3d_dgrad calls through `res`). */
int ru3d_conv3d_s2_dgrad_pair_supported(const ru3d_tensor* dy, const ru3d_tensor* dy2, const ru3d_tensor* res,
                                        const ru3d_tensor* dx, int dtype);
int ru3d_conv3d_s2_dgrad_pair(const ru3d_tensor* dy, const void* w3_packed, const ru3d_tensor* dy2,
                              const void* w1_packed, const ru3d_tensor* res, const ru3d_tensor* dx, int dtype,
                              void* stream);
/* weight gradient, written as fp32 in the reference layout [Cout][Cin][k^3] (param.grad). */
size_t ru3d_conv3d_wgrad_workspace_bytes(const ru3d_tensor* x, const ru3d_tensor* dy, int k, int stride, int dtype);
int ru3d_conv3d_wgrad(const ru3d_tensor* x, const ru3d_tensor* dy, float* dw, void* ws, size_t ws_bytes,
                      int k, int stride, int dtype, void* stream);

/* A ResBlock's two weight gradients on its input x (reference network.py:403-409: conv1 3x3x3 and skip_conv 1x1x1, both
 * with the block's stride 1 or 2, on the same x) from ONE pass over x:  dw[Cout][Cin][27] = wgrad3(x, dy),
 * dw2[Cout][Cin] = wgrad1(x, dy2).  dy and dy2 have the same shape.  x may be a split tensor (stride 1).  Ask _supported
 * first (the sliding / LDS-DMA weight-gradient kernels' shapes, 16-bit storage); workspace: _workspace_bytes. */
int ru3d_conv3d_wgrad_pair_supported(const ru3d_tensor* x, const ru3d_tensor* dy, const ru3d_tensor* dy2, int stride, int dtype);
size_t ru3d_conv3d_wgrad_pair_workspace_bytes(const ru3d_tensor* x, const ru3d_tensor* dy, const ru3d_tensor* dy2, int stride,
                                              int dtype);
int ru3d_conv3d_wgrad_pair(const ru3d_tensor* x, const ru3d_tensor* dy, const ru3d_tensor* dy2, float* dw, float* dw2,
                           void* ws, size_t ws_bytes, int stride, int dtype, void* stream);
/* The same weight gradient AND the conv's bias gradient db[co] = sum over samples and voxels of dy (autograd of the bias of
 * network.py:541 conv / any nn.Conv3d) behind one entry point: the stem's MFMA kernel delivers db from its own pass over dy
 * (an extra all-ones row of its im2col operand); other shapes run ru3d_conv3d_wgrad + ru3d_channel_sum. */
size_t ru3d_conv3d_wgrad_bias_workspace_bytes(const ru3d_tensor* x, const ru3d_tensor* dy, int k, int stride, int dtype);
int ru3d_conv3d_wgrad_bias(const ru3d_tensor* x, const ru3d_tensor* dy, float* dw, float* db, void* ws, size_t ws_bytes,
                           int k, int stride, int dtype, void* stream);
/* The whole backward of the 1x1x1 head conv (network.py:547 `fc`, Cout <= 4) in one pass: x = the head's input (16-bit
 * storage), dlogits = the loss's gradient as fp32 [N][D][H][W][Cout] (it is rounded to the storage type in registers, the
 * value the unfused path's cast stored), weight = the fp32 parameter [Cout][cin_real] (cin_real < x->c: padded channels),
 * -> dx (storage type, pad lanes 0), dw [Cout][cin_real], db [Cout] (may be NULL). */
int ru3d_head_bwd_supported(const ru3d_tensor* x, const ru3d_tensor* dlogits, const ru3d_tensor* dx, int dtype);
size_t ru3d_head_bwd_workspace_bytes(const ru3d_tensor* x, int dtype);
int ru3d_head_bwd(const ru3d_tensor* x, const ru3d_tensor* dlogits, const float* weight, int cin_real, const ru3d_tensor* dx,
                  float* dw, float* db, void* ws, size_t ws_bytes, int dtype, void* stream);
/* ru3d_head_bwd followed by ru3d_in_lrelu_bwd(gpre, gpre_sum) for a head whose input is a residual block's output
 * z = LeakyReLU((y - mean) * scale + skip), without the head's input gradient dz ever reaching memory: dw and db come from
 * ru3d_head_bwd's pass over (z, dlogits) without its store, and the reduction pass of the InstanceNorm backward forms dz
 * in registers from dlogits and the weight instead of reading it (it reads z, y, dlogits and writes gpre = dz *
 * LeakyReLU'(z)); finalize and apply follow as in ru3d_in_lrelu_bwd.  Grids, voxel orders and summation orders are the
 * two calls': gpre, dy, dw, db and gpre_sum (optional, C floats) are bit for bit theirs.  `_supported`:
 * ru3d_head_bwd's conditions, 16-byte rows, and a level ru3d_in_lrelu_bwd runs as three launches (not the small-level
 * kernels). */
int ru3d_head_in_bwd_supported(const ru3d_tensor* z, const ru3d_tensor* dlogits, const ru3d_tensor* y,
                               const ru3d_tensor* gpre, const ru3d_tensor* dy, int dtype);
size_t ru3d_head_in_bwd_workspace_bytes(const ru3d_tensor* z, int dtype);
int ru3d_head_in_bwd(const ru3d_tensor* z, const ru3d_tensor* dlogits, const float* weight, int cin_real,
                     const ru3d_tensor* y, const float* mean, const float* scale, const ru3d_tensor* gpre,
                     const ru3d_tensor* dy, float* dw, float* db, float* gpre_sum, void* ws, size_t ws_bytes, float slope,
                     int dtype, void* stream);

/* nn.ConvTranspose3d(k3,s2,p1) followed by ConstantPad3d((0,1,0,1,0,1),0) (network.py:312-314):
 * y has extents 2*x.{d,h,w}; its far planes are written as exact zeros (no bias there). */
int ru3d_convtranspose3d_k3s2p1_fwd(const ru3d_tensor* x, const void* w_packed, const float* bias,
                                    const ru3d_tensor* y, int dtype, void* stream);
/* The same followed by the InstanceNorm statistics of y (network.py:315; the zero far planes count): mean / scale as
 * ru3d_instnorm_stats writes them; fused into the transposed conv's epilogue where a kernel for the shape exists. */
size_t ru3d_convtranspose3d_k3s2p1_fwd_in_workspace_bytes(const ru3d_tensor* x, const ru3d_tensor* y, int dtype);
int ru3d_convtranspose3d_k3s2p1_fwd_in(const ru3d_tensor* x, const void* w_packed, const float* bias,
                                       const ru3d_tensor* y, float* mean, float* scale, void* ws, size_t ws_bytes,
                                       float eps, int dtype, void* stream);
/* dy must have zero far planes (ru3d_in_lrelu_bwd(zero_far=1) guarantees it). */
int ru3d_convtranspose3d_k3s2p1_dgrad(const ru3d_tensor* dy, const void* w_packed, const ru3d_tensor* dx,
                                      int dtype, void* stream);
size_t ru3d_convtranspose3d_k3s2p1_wgrad_workspace_bytes(const ru3d_tensor* x, const ru3d_tensor* dy, int dtype);
/* dw fp32 in the reference layout [Cin][Cout][27]. */
int ru3d_convtranspose3d_k3s2p1_wgrad(const ru3d_tensor* x, const ru3d_tensor* dy, float* dw, void* ws,
                                      size_t ws_bytes, int dtype, void* stream);

/* ------------------------------------------------------------------ InstanceNorm + LeakyReLU - */
size_t ru3d_reduce_workspace_bytes(const ru3d_tensor* t);
/* nn.InstanceNorm3d(eps, affine=False) statistics (network.py:401,414), with the preceding
 * nn.Dropout3d folded in: drop_scale[n*C+c] in {0, 1/(1-p)} or NULL.
 * Outputs mean[n*C+c] of the raw y and scale = s / sqrt(s^2 * var + eps), so that
 * x_hat = (y - mean) * scale equals InstanceNorm(Dropout3d(y)). */
int ru3d_instnorm_stats(const ru3d_tensor* y, const float* drop_scale, float* mean, float* scale,
                        void* ws, size_t ws_bytes, float eps, int dtype, void* stream);
/* The tail of a decoder ResBlock in one pass (network.py:403, 406-409, 414-416): out = LeakyReLU((y - mean) * scale +
 * conv1x1(x; w_packed, bias), slope) - the skip conv's output is never stored.  `_supported`: a kernel exists for the
 * shapes (the caller otherwise runs ru3d_conv3d_fwd(k = 1) + ru3d_in_lrelu_fwd(res = skip)). */
int ru3d_skip1x1_in_lrelu_fwd_supported(const ru3d_tensor* x, const ru3d_tensor* y, const ru3d_tensor* out, int dtype);
int ru3d_skip1x1_in_lrelu_fwd(const ru3d_tensor* x, const void* w_packed, const float* bias, const ru3d_tensor* y,
                              const float* mean, const float* scale, const ru3d_tensor* out, float slope, int dtype,
                              void* stream);
/* The same pass when `out` feeds only the network's 1x1x1 head (network.py:547 `fc`, Cout <= 4, Cin = out->c): the
 * head's fp32 logits [N][D][H][W][Cout] are formed from the stored (rounded) `out` in the kernel's epilogue, bit for bit
 * what ru3d_conv3d_fwd(k = 1) on `out` gives; `out` is still written.  head_w_packed: the head's forward pack
 * ([cin][cout_pad = 4]); head_bias: fp32 [Cout] or NULL. */
int ru3d_skip1x1_in_lrelu_head_fwd_supported(const ru3d_tensor* x, const ru3d_tensor* y, const ru3d_tensor* out,
                                             const ru3d_tensor* logits, int dtype);
int ru3d_skip1x1_in_lrelu_head_fwd(const ru3d_tensor* x, const void* w_packed, const float* bias, const ru3d_tensor* y,
                                   const float* mean, const float* scale, const ru3d_tensor* out, const void* head_w_packed,
                                   const float* head_bias, const ru3d_tensor* logits, float slope, int dtype, void* stream);
/* out = LeakyReLU((y - mean) * scale (+ res), slope)  (network.py:414,416; 315-316). */
int ru3d_in_lrelu_fwd(const ru3d_tensor* y, const float* mean, const float* scale, const ru3d_tensor* res,
                      const ru3d_tensor* out, float slope, int dtype, void* stream);
/* backward of the above: given gout = dL/dout, writes dy = dL/dy and, when the forward had a residual,
 * gpre = gout * LeakyReLU'(out) = dL/dres.  CONTRACT: gpre != NULL <=> the forward was called with a residual.
 * Without a residual out = LeakyReLU(x_hat) is invertible, so x_hat is recovered from `out` and `y` is not
 * read at all (one tensor pass less in each of the two kernels).  zero_far=1 additionally zeroes the last plane
 * of each spatial axis of dy (the constant-pad planes of ConvTrans3D).
 * gpre_sum (optional, C floats): sum over n and voxels of gpre - the bias gradient of a conv that feeds the
 * residual input (skip_conv, network.py:407-409); it falls out of the reduction this call runs anyway.
 * dy_sum (optional, C floats): sum over n and voxels of the stored dy - the bias gradient of the conv or transposed
 * conv that produced y (network.py:290-300); per-block sums in the epilogue of the pass that writes dy. */
int ru3d_in_lrelu_bwd(const ru3d_tensor* gout, const ru3d_tensor* out, const ru3d_tensor* y, const float* mean,
                      const float* scale, const ru3d_tensor* dy, const ru3d_tensor* gpre, void* ws,
                      size_t ws_bytes, float slope, int zero_far, float* gpre_sum, float* dy_sum, int dtype,
                      void* stream);
/* out[c] = sum over n,d,h,w of t (bias gradients). */
int ru3d_channel_sum(const ru3d_tensor* t, float* out, void* ws, size_t ws_bytes, int dtype, void* stream);
/* nn.Dropout3d(p) channel mask (network.py:397-398,412-413): scale[n*C+c] = keep ? 1/(1-p) : 0,
 * counter-based RNG keyed by (seed, offset). */
int ru3d_dropout3d_scale(float* scale, int count, float p, uint64_t seed, uint64_t offset, void* stream);
/* The same draw with the counter offset completed ON THE DEVICE: offset + *offset_base.  For a training step captured
 * in a hipGraph - the launch arguments are frozen at capture; the host advances *offset_base between replays, so replay
 * k draws exactly the masks the eager step k would have drawn. */
int ru3d_dropout3d_scale_dev(float* scale, int count, float p, uint64_t seed, uint64_t offset,
                             const uint64_t* offset_base, void* stream);

/* Elementwise pieces of the attention gate (AttBlock, network.py:353-371: x = conv(x); g = conv(gate);
 * rate = sigmoid(conv(lrelu(x + g))); return x * rate) and of its backward; the convolutions are ru3d_conv3d_*.
 *   op 0: o1 = lrelu(a)                                  op 1: o1 = a * sigmoid(b)
 *   op 2: o1 = c * sigmoid(b),  o2 = c * a * sigmoid'(b)  (c = upstream gradient, a = gated tensor, b = pre-sigmoid)
 *   op 3: o1 = c * lrelu'(a),   o2 = o1 + b               (a = the lrelu OUTPUT, c = its gradient, b = another share) */
int ru3d_pointwise(int op, const ru3d_tensor* a, const ru3d_tensor* b, const ru3d_tensor* c, const ru3d_tensor* o1,
                   const ru3d_tensor* o2, float slope, int dtype, void* stream);

/* ------------------------------------------------------------------ layout helpers ---------- */
/* dst[...,c] = src[...,c] for c < src.c (torch.cat along channels, network.py:350, written in place). */
int ru3d_copy_channels(const ru3d_tensor* src, const ru3d_tensor* dst, int dtype, void* stream);
/* dst = src + add, same shape (gradient accumulation of the skip branch). */
int ru3d_add(const ru3d_tensor* a, const ru3d_tensor* b, const ru3d_tensor* dst, int dtype, void* stream);
/* 2x2x2 / stride-2 max pooling (MaxPoolBlock, network.py:452-463: nn.MaxPool3d(2, 2)); dtype: any of the three storage
 * types (the values are copied, never rounded).  Any c; odd spatial extents are floored, an extent below 2 is an error;
 * a split tensor is rejected.
 * y[n,c,od,oh,ow] = max over the 2x2x2 window of x at (2od.., 2oh.., 2ow..), a bit copy of the element that wins by torch's
 * rule: scan in (d, h, w) order, replace the running maximum when v > max || isnan(v) (first of equals, the last NaN).
 * idx (may be NULL: inference) receives one byte per element of y, dense NDHWC in y's logical shape: code = dz*4 + dy*2 +
 * dx of the element that won. */
int ru3d_maxpool3d_fwd(const ru3d_tensor* x, const ru3d_tensor* y, uint8_t* idx, int dtype, void* stream);
/* dx = the gradient of the above: dy at the winning element of each window, 0 elsewhere, 0 in the trailing planes of odd
 * extents.  Writes EVERY element of dx. */
int ru3d_maxpool3d_bwd(const ru3d_tensor* dy, const uint8_t* idx, const ru3d_tensor* dx, int dtype, void* stream);
/* dst (dtype `dst_dtype`) = src (fp32), same shape: fp32 logits-gradient -> storage dtype. */
int ru3d_cast_f32(const ru3d_tensor* src, const ru3d_tensor* dst, int dst_dtype, void* stream);
/* NCDHW fp32 (reference tensor layout) -> NDHWC `dtype`, and back. */
int ru3d_ncdhw_to_ndhwc(const float* src, const ru3d_tensor* dst, int dtype, void* stream);
int ru3d_ndhwc_to_ncdhw(const ru3d_tensor* src, float* dst, int dtype, void* stream);

/* ------------------------------------------------------------------ loss -------------------- */
/* Fused softmax + focal + Tversky sums (loss.py:7-48, 51-82, 218-254): one pass over logits+labels.
 * logits: fp32, element (n, c, v) at logits[n*stride_n + c*stride_c + v*stride_v] (covers both the
 * NDHWC tensor the network writes and a plain NCDHW tensor).  labels: [N*V] int64 or uint8.
 * state: caller-owned device buffer of ru3d_loss_state_bytes(C) bytes; receives the class sums, the
 * backward coefficients and the number of out-of-range labels.  loss_out: 1 fp32 on device.
 * C == 1 uses sigmoid with an all-ones one-hot (what F.one_hot(target, 1) yields for valid targets). */
size_t ru3d_loss_state_bytes(int num_classes);
/* byte offset, inside the state buffer, of the int32 count of labels outside [0, C) that the forward pass found (the
 * reference's F.one_hot raises for them, loss.py:27): a host can read these 4 bytes at its next read-back. */
size_t ru3d_loss_state_bad_labels_offset(void);
size_t ru3d_loss_workspace_bytes(int n, int64_t v, int num_classes);
int ru3d_loss_fwd(const float* logits, int64_t stride_n, int64_t stride_c, int64_t stride_v, const void* labels,
                  int label_dtype, int n, int64_t v, int num_classes, int kind, float gamma, const float* weight_v,
                  float alpha, float beta, float smooth, void* state, float* loss_out, void* ws, size_t ws_bytes,
                  void* stream);
/* dlogits (same strides as logits; dtype f32 or bf16) = grad_out[0] * dLoss/dlogits. */
int ru3d_loss_bwd(const float* logits, int64_t stride_n, int64_t stride_c, int64_t stride_v, const void* labels,
                  int label_dtype, int n, int64_t v, int num_classes, float gamma, const void* state,
                  const float* grad_out, void* dlogits, int dlogits_dtype, void* stream);
/* Ignore label of the softmax losses: train on partly annotated cases.  ru3d_loss_ignore_fwd / _bwd,
 * ru3d_ds_loss_ignore_fwd / _bwd and ru3d_topk_loss_ignore_fwd / _bwd are their namesakes with (has_ignore, ignore_label)
 * behind num_classes, as ru3d_group_loss_fwd takes them; the plain entry points are calls of these with has_ignore = 0,
 * which launch the same kernels on the same arithmetic as before.  State sizes, workspace sizes and the bad-label offset
 * functions are shared.  has_ignore != 0 selects kernels instantiated for it (no run-time branch in the plain ones).
 * The loss with an ignore label is the loss of the counted voxels alone.  Let S be the voxels with
 * t_v != ignore_label - over the whole batch, as all sums of these losses are - and M = |S|:
 *   tp_c, sp_c, sg_c run over S only (an ignored voxel adds to no sum, not to sp either); the Tversky formula is unchanged.
 *   focal_c = C * (sum over S of -(1-p_c)^gamma g_c log p_c) / max(M, 1): the "C * mean over all rows" of the rows that
 *     remain.  M is sum_c sg_c, float64 sums of exact small integers: the state keeps its layout.
 *   d loss / d logits is exactly 0.0 at every ignored voxel, in every class channel: the backward writes these zeros.
 *   The label is loaded first and an ignored voxel's logits are never read: NaN or Inf there leaves the loss finite and
 *     every other gradient unchanged.
 *   M = 0 gives dice_c = (0 + s) / (0 + s) = 1: DiceLoss 0, FocalLoss 0, HybirdLoss 0, Dice sum w; gradient all zeros.
 *   A label outside [0, C) that is not the ignore label is a bad label as before: counted, loss NaN.
 *   Deep supervision: a level's voxel is ignored iff the label it reads is the ignore label; every level has its own
 *     M_l and its own max(M_l, 1).
 *   Top-k (nnU-Net's ignore_index rule): an ignored voxel has ce = 0 and takes part in the selection like any voxel whose
 *     cross-entropy is 0; K stays the caller's launch argument, relative to all n * v voxels; the ignored voxels get a zero
 *     gradient whatever share the tie rule gives to voxels at ce == tau == 0; the Dice leg follows the rule above.
 * Refused before any launch, like every argument error: an ignore_label inside [0, C); C == 1 (the sigmoid form has the
 * all-ones one-hot quirk; the group loss is the single-channel loss with an ignore label); uint8 labels with an
 * ignore_label outside 0 .. 255.  With int64 labels any int value outside [0, C) is legal, e.g. -1 or 255. */
int ru3d_loss_ignore_fwd(const float* logits, int64_t stride_n, int64_t stride_c, int64_t stride_v, const void* labels,
                         int label_dtype, int n, int64_t v, int num_classes, int has_ignore, int ignore_label, int kind,
                         float gamma, const float* weight_v, float alpha, float beta, float smooth, void* state,
                         float* loss_out, void* ws, size_t ws_bytes, void* stream);
int ru3d_loss_ignore_bwd(const float* logits, int64_t stride_n, int64_t stride_c, int64_t stride_v, const void* labels,
                         int label_dtype, int n, int64_t v, int num_classes, int has_ignore, int ignore_label,
                         float gamma, const void* state, const float* grad_out, void* dlogits, int dlogits_dtype,
                         void* stream);
/* functional `dice` of loss.py:32-48 on two flat fp32 vectors (used by trainer.evaluate_case). */
int ru3d_tversky(const float* p, const float* g, int64_t count, float alpha, float beta, float smooth,
                 float* out, void* ws, size_t ws_bytes, void* stream);

/* ------------------------------------------------------------------ sliding-window inference */
/* predict_per_patch (trainer.py:17-98).  `acc` is a zero-initialised [X, Y, Z, C] fp32 volume, `cnt` a
 * zero-initialised [X, Y, Z] fp32 volume (the reference's `result` / `result_n`, trainer.py:42-43).
 * accumulate: acc[window] += softmax_c(logits[sample]) (sigmoid when C == 1), cnt[window] += 1, the window
 * being [ox, ox+d) x [oy, oy+h) x [oz, oz+w) (trainer.py:72-80).  Launches for overlapping windows must be
 * issued on one stream; the sum order is then the launch order, as in the reference's patch loop. */
int ru3d_predict_accumulate(const ru3d_tensor* logits, int dtype, int sample, float* acc, float* cnt, int X, int Y,
                            int Z, int ox, int oy, int oz, void* stream);
/* merge (trainer.py:85-98) over the crop [cx, cx+sx) x [cy, cy+sy) x [cz, cz+sz) of the padded volume:
 * one_hot != 0: out = float [sx, sy, sz, C] = acc / cnt (NaN where no window reached, as in the reference);
 * one_hot == 0: out = uint8 [sx, sy, sz]: C == 1 -> round(acc / cnt); C > 1 -> argmax_c softmax_c(acc / cnt)
 * (the reference's second softmax); uncovered voxels -> 0. */
int ru3d_predict_merge(const float* acc, const float* cnt, int X, int Y, int Z, int num_classes, int cx, int cy,
                       int cz, int sx, int sy, int sz, int one_hot, void* out, void* stream);
/* Mirrored / weighted / ensemble sliding windows (inference.py: placement, weighting, mirror_axes, model lists).
 * A mirror mask has bit 0 for the volume's X axis, bit 1 for Y, bit 2 for Z.
 * gather: one launch fills the whole model input.  vol is the padded volume, fp32 [X, Y, Z, cin]; dst the dense NDHWC
 * fp32 activation [count, px, py, pz, cin]; `windows` is a HOST array of 4 * count int32 (ox, oy, oz, mirror mask) per
 * batch entry, copied into the launch arguments (count <= RU3D_PREDICT_MAX_BATCH; more is refused):
 *     dst[b][a][j][k][c] = vol[ox_b + a'][oy_b + j'][oz_b + k'][c],  a' = px-1-a where bit 0 of the mask is set, else a
 * (likewise j', k'), i.e. torch.flip of the window along the masked axes. */
#define RU3D_PREDICT_MAX_BATCH 16
int ru3d_predict_gather(const float* vol, int X, int Y, int Z, int cin, const int32_t* windows, int count,
                        const ru3d_tensor* dst, void* stream);
/* accumulate_weighted: as accumulate, for logits the model computed on a window mirrored by `flip`: the probabilities
 * are mirrored back (read at the mirrored index), multiplied by (gx[a] * gy[j]) * gz[k] in fp32 - three DEVICE tables
 * of d, h and w floats indexed by the voxel's place in the window, all three NULL for weight 1 - and added into acc;
 * the weight is added into cnt, so merge stays acc / cnt.  No atomics: one thread owns a voxel of the window, launches
 * on one stream sum in launch order, and the result does not depend on how windows were batched.  With flip 0 and
 * NULL tables the sums are bit-identical to accumulate's.  Same argument checks, refused before launch. */
int ru3d_predict_accumulate_weighted(const ru3d_tensor* logits, int dtype, int sample, int flip, const float* gx,
                                     const float* gy, const float* gz, float* acc, float* cnt, int X, int Y, int Z,
                                     int ox, int oy, int oz, void* stream);

/* ------------------------------------------------------------------ overlapping label groups */
/* One sigmoid channel per GROUP of label values (csrc/groups.hip); groups may overlap, e.g. ((1, 2), (2,)) = whole
 * kidney, tumour.  `table` is a HOST array of num_labels bytes, copied into the launch arguments: bit k of table[t] is
 * set iff label value t is a member of group k (num_groups 1..8, num_labels 1..32).  The target of channel k at a voxel
 * with label t is that bit; no multi-hot tensor exists.  has_ignore != 0: voxels whose label equals ignore_label (which
 * must lie outside [0, num_labels)) enter no sum and get a zero gradient in every channel; M counts the others.  Any
 * other label outside [0, num_labels) is a bad label: all channels off, counted in the state block, loss NaN.
 * Over the counted voxels, p = sigmoid(z_k), g the target:
 *   dice_k  = (tp + s) / (tp + alpha (sg - tp) + beta (sp - tp) + s),  tp = sum p g, sp = sum p, sg = sum g
 *   focal_k = 1 / max(M, 1) sum [ (1-p)^gamma g softplus(-z) + p^gamma (1-g) softplus(z) ]   (gamma 0: binary CE)
 *   w = weight_v / sum|weight_v| (HOST array of num_groups floats or NULL = ones), kind as ru3d_loss_fwd:
 *   HYBIRD sum w (1 - dice + focal), DICELOSS sum w (1 - dice), FOCAL sum w focal, DICE sum w dice.
 * Operands otherwise as ru3d_loss_fwd / ru3d_loss_bwd: fp32 logits with (stride_n, stride_c, stride_v), int64 or uint8
 * labels, state of ru3d_group_loss_state_bytes() bytes - it begins like the state of ru3d_loss_fwd, so the bad-label
 * count sits at ru3d_loss_state_bad_labels_offset() -, loss_out 1 fp32 on the device, dlogits f32 or bf16 with the
 * logits' strides.  One pass each, fixed-order reductions, no atomics, no host synchronisation: bit-reproducible.
 * Every argument error is refused before any launch. */
size_t ru3d_group_loss_state_bytes(void);
size_t ru3d_group_loss_workspace_bytes(int n, int64_t v, int num_groups);
int ru3d_group_loss_fwd(const float* logits, int64_t stride_n, int64_t stride_c, int64_t stride_v, const void* labels,
                        int label_dtype, int n, int64_t v, int num_groups, const uint8_t* table, int num_labels,
                        int has_ignore, int ignore_label, int kind, float gamma, const float* weight_v, float alpha,
                        float beta, float smooth, void* state, float* loss_out, void* ws, size_t ws_bytes, void* stream);
int ru3d_group_loss_bwd(const float* logits, int64_t stride_n, int64_t stride_c, int64_t stride_v, const void* labels,
                        int label_dtype, int n, int64_t v, int num_groups, const uint8_t* table, int num_labels,
                        int has_ignore, int ignore_label, float gamma, const void* state, const float* grad_out,
                        void* dlogits, int dlogits_dtype, void* stream);
/* ------------------------------------------------------------------ top-k cross-entropy */
/* ru3d_topk_select: exact top-K statistics of n finite device floats (csrc/topk.hip), 1 <= K <= n.  *result (device):
 * tau = the K-th largest value, count_gt = #{x > tau}, count_eq = #{x == tau}, sum_gt = the sum of the values above tau,
 * accumulated in float64 from the element on (per-workgroup partial rows added in a fixed order: the same bits every
 * run).  The two zeros are one value and a zero tau is +0.  mean of the K largest = (sum_gt + (K - count_gt) * tau) / K.
 * Radix select with 11 / 11 / 10-bit digits: the values are read three times, never moved (what lies above tau in the
 * last digit is summed from that digit's table); no host synchronisation, capturable.  ru3d_topk_select_trip_elements(): the values one grid-stride trip of its largest grid covers. */
typedef struct ru3d_topk_result {
    float tau;
    int64_t count_gt;
    int64_t count_eq;
    double sum_gt;
} ru3d_topk_result;
size_t ru3d_topk_select_workspace_bytes(int64_t n);
int64_t ru3d_topk_select_trip_elements(void);
int ru3d_topk_select(const float* values, int64_t n, int64_t K, ru3d_topk_result* result, void* ws, size_t ws_bytes,
                     void* stream);
/* Top-k cross-entropy loss, alone (with_dice == 0: loss.TopKLoss, ce_weight scales it) or added to DiceLoss's region term
 * (with_dice != 0: loss.HybirdTopKLoss).  With ce_v = -log softmax(z_v)[t_v] in float32 over the M = n * v voxels of the
 * batch, tau their K-th largest, G = #{ce > tau}, E = #{ce == tau}:
 *   topk = (sum_{ce > tau} ce + (K - G) * tau) / K                  (= torch.topk(ce, K).values.mean())
 *   loss = [sum_c w_c (1 - dice_c)] + ce_weight * topk,  w and the Tversky dice_c as ru3d_loss_fwd's RU3D_LOSS_DICELOSS
 *   d topk / d z_{v,c} = s_v (p_{v,c} - [c == t_v]) / K,  s_v = 1 if ce_v > tau, (K - G) / E if ce_v == tau, else 0
 * (voxels tied at the threshold share the remaining weight equally).  Operands as ru3d_loss_fwd / ru3d_loss_bwd, with
 * 2 <= num_classes <= 8 and 1 <= K <= M.  ce: caller-owned device float32 [M], written by the forward and read by the
 * backward, which compares the stored values with tau: it must not be touched in between.  state: device buffer of
 * ru3d_topk_loss_state_bytes() bytes; it begins like the state of ru3d_loss_fwd (the bad-label count sits at
 * ru3d_loss_state_bad_labels_offset()) and continues with tau (float32, 4 bytes of padding), G, E, K as int64 and the two
 * backward weights ce_weight / K and ce_weight (K - G) / (E K) as float32.  A label outside [0, C) is counted, its ce is 0 and the loss is NaN.
 * The forward reads logits and labels once and ce[] twice; no host synchronisation, capturable; K is a launch
 * argument.  ru3d_topk_loss_fwd_timed (tools): the same forward with an event after every launch; it waits for the stream
 * and writes the milliseconds of the ru3d_topk_loss_fwd_launches() launches to the HOST array launch_ms. */
size_t ru3d_topk_loss_state_bytes(void);
size_t ru3d_topk_loss_workspace_bytes(int n, int64_t v, int num_classes);
int ru3d_topk_loss_fwd(const float* logits, int64_t stride_n, int64_t stride_c, int64_t stride_v, const void* labels,
                       int label_dtype, int n, int64_t v, int num_classes, int64_t K, int with_dice,
                       const float* weight_v, float alpha, float beta, float smooth, float ce_weight, float* ce,
                       void* state, float* loss_out, void* ws, size_t ws_bytes, void* stream);
int ru3d_topk_loss_fwd_launches(void);
int ru3d_topk_loss_fwd_timed(const float* logits, int64_t stride_n, int64_t stride_c, int64_t stride_v, const void* labels,
                             int label_dtype, int n, int64_t v, int num_classes, int64_t K, int with_dice,
                             const float* weight_v, float alpha, float beta, float smooth, float ce_weight, float* ce,
                             void* state, float* loss_out, void* ws, size_t ws_bytes, float* launch_ms, void* stream);
int ru3d_topk_loss_bwd(const float* logits, int64_t stride_n, int64_t stride_c, int64_t stride_v, const void* labels,
                       int label_dtype, int n, int64_t v, int num_classes, int with_dice, const float* ce,
                       const void* state, const float* grad_out, void* dlogits, int dlogits_dtype, void* stream);
/* the same with an ignore label (semantics: the comment of ru3d_loss_ignore_fwd) */
int ru3d_topk_loss_ignore_fwd(const float* logits, int64_t stride_n, int64_t stride_c, int64_t stride_v,
                              const void* labels, int label_dtype, int n, int64_t v, int num_classes, int has_ignore,
                              int ignore_label, int64_t K, int with_dice, const float* weight_v, float alpha, float beta,
                              float smooth, float ce_weight, float* ce, void* state, float* loss_out, void* ws,
                              size_t ws_bytes, void* stream);
int ru3d_topk_loss_ignore_bwd(const float* logits, int64_t stride_n, int64_t stride_c, int64_t stride_v,
                              const void* labels, int label_dtype, int n, int64_t v, int num_classes, int has_ignore,
                              int ignore_label, int with_dice, const float* ce, const void* state, const float* grad_out,
                              void* dlogits, int dlogits_dtype, void* stream);
/* accumulate_groups: signature and contract of ru3d_predict_accumulate_weighted (flip, three device tables that may all
 * be NULL, one thread per window voxel, sums in launch order) with an independent sigmoid per channel in place of the
 * softmax; f32 or bf16 logits of 1..8 channels.  With flip 0 and NULL tables it serves the reference placement too. */
int ru3d_predict_accumulate_groups(const ru3d_tensor* logits, int dtype, int sample, int flip, const float* gx,
                                   const float* gy, const float* gz, float* acc, float* cnt, int X, int Y, int Z,
                                   int ox, int oy, int oz, void* stream);
/* merge_groups: uint8 [sx, sy, sz] over the crop, as ru3d_predict_merge takes it.  group_labels and threshold are HOST
 * arrays of num_groups values (labels 0..255), copied into the launch arguments.  Channel k is on iff
 * acc_k / cnt > threshold[k]; the voxel gets group_labels[k] of the LAST channel that is on (later groups overwrite
 * earlier ones), 0 when none is, when cnt == 0 or when the mean is NaN.  The mean probabilities themselves are
 * ru3d_predict_merge(..., one_hot = 1). */
int ru3d_predict_merge_groups(const float* acc, const float* cnt, int X, int Y, int Z, int num_groups,
                              const int32_t* group_labels, const float* threshold, int cx, int cy, int cz, int sx,
                              int sy, int sz, uint8_t* out, void* stream);

/* ------------------------------------------------------------------ connected components + cascade merge */
/* 3D connected-component labelling with 6-connectivity, scipy.ndimage.label's default structure (transform.py:5-11,
 * data.py:464-492).  mask: uint8 [X, Y, Z], Z contiguous, any non-zero byte is foreground.  labels: int32 [X, Y, Z],
 * 0 on background and 1..K on foreground, the components numbered by the linear index of their first voxel - scipy's
 * numbering, element for element.  K is written to *count_dev (device int32).  Integer atomics only: the result is a
 * pure function of the mask.  X*Y*Z must stay below 2^31.  `ws`: device scratch of the size the query returns. */
size_t ru3d_components_workspace_bytes(int X, int Y, int Z);
int ru3d_label_components(const uint8_t* mask, int X, int Y, int Z, int32_t* labels, int32_t* count_dev, void* ws,
                          size_t ws_bytes, void* stream);
/* sizes[k] (int32) = voxels of component k + 1, boxes[k] (int32[6]) = {x0, x1, y0, y1, z0, z1} with x1 = last x + 1
 * (np.bincount(labels)[1:] and scipy.ndimage.find_objects).  `count` = K, read back by the caller. */
int ru3d_component_stats(const int32_t* labels, int X, int Y, int Z, int count, int32_t* sizes, int32_t* boxes,
                         void* stream);
/* remove_small_region (transform.py:5-11): components with sizes[k] < threshold are zeroed in mask_inout (uint8, may
 * be NULL) and the survivors renumbered 1..kept in their old order into labels_out (int32, may be NULL, may be
 * `labels` itself) - what a second labelling of the filtered mask would return.  *kept_dev (device int32) = kept. */
size_t ru3d_filter_components_workspace_bytes(int count);
int ru3d_filter_components(const int32_t* labels, int X, int Y, int Z, int count, const int32_t* sizes, int threshold,
                           uint8_t* mask_inout, int32_t* labels_out, int32_t* kept_dev, void* ws, size_t ws_bytes,
                           void* stream);
/* Keep the k largest components (1 <= k <= RU3D_KEEP_LARGEST_MAX): one workgroup picks them from sizes[0 .. count) on
 * the device - among equal sizes the smaller component number wins, np.argsort(-sizes, kind='stable')[:k] - and the
 * pass of ru3d_filter_components zeroes the others in mask_inout and / or renumbers the survivors in their old order
 * into labels_out, with the same rules for NULL and for labels_out == labels.  k >= count keeps everything.  No size
 * crosses to the host.  *kept_dev (device int32) = min(k, count).  `ws`: as for ru3d_filter_components, sized by
 * ru3d_filter_components_workspace_bytes(count) - the call uses its renumbering table. */
#define RU3D_KEEP_LARGEST_MAX 8
int ru3d_keep_largest_components(const int32_t* labels, int X, int Y, int Z, int count, const int32_t* sizes, int k,
                                 uint8_t* mask_inout, int32_t* labels_out, int32_t* kept_dev, void* ws, size_t ws_bytes,
                                 void* stream);
/* cascade_predict_case (trainer.py:203-240).  total: zero-initialised float64 [X, Y, Z, C], hits: zero-initialised
 * int32 [X, Y, Z] (the reference's C copies of `hits` are equal).  accumulate: prob is one region's float32
 * [rx, ry, rz, C] map whose box starts at (bx, by, bz) in volume coordinates (negative where the padded box leaves the
 * volume); the part inside the volume is added to `total` and counted in `hits`.  Regions that overlap must be
 * accumulated on one stream; the sum order is then the launch order, as in the reference's region loop.
 * merge: out (uint8 [X, Y, Z]) = total / hits where hits > 0, then round half to even for C == 1, argmax_c softmax_c
 * with the first maximum winning for C > 1; a row holding a NaN gives 0.  All arithmetic in float64. */
int ru3d_region_accumulate(const float* prob, int rx, int ry, int rz, int num_classes, int bx, int by, int bz,
                           double* total, int32_t* hits, int X, int Y, int Z, void* stream);
int ru3d_cascade_merge(const double* total, const int32_t* hits, int X, int Y, int Z, int num_classes, uint8_t* out,
                       void* stream);

/* ------------------------------------------------------------------ morphometry of a label volume */
/* What a report says about every structure (csrc/morphometry.hip).  ids: a uint8 class volume (id_bytes = 1) or an
 * int32 component-label volume (id_bytes = 4), [X, Y, Z] with Z contiguous, X*Y*Z < 2^31, any alignment.  Ids
 * 1 .. count are measured; 0 and every value above `count` (a stray 255 ignore label) is skipped silently.  Every
 * output is written in full by the call, whatever it held before, and nothing but the outputs is written; no entry
 * point needs scratch.  Integer atomics and 64-bit min / max only: exact, and the same bytes in every run.  count = 0
 * launches nothing.  The grids are sized by ru3d_get_cu_budget().
 *
 * moments: table (int64 [count][10]) = n, Sx, Sy, Sz, Sxx, Syy, Szz, Sxy, Sxz, Syz over the voxel indices of each id.
 * Refused when X*Y*Z * (largest extent - 1)^2 reaches 2^63. */
int ru3d_label_moments(const void* ids, int id_bytes, int X, int Y, int Z, int count, int64_t* table, void* stream);
/* faces: other is a uint8 volume over the same grid with classes 0 .. num_other - 1 (num_other <= 256).  table (int64
 * [count][num_other + 1][3]): for every voxel p of id k and each of its six neighbours q, a q outside the volume counts
 * in column num_other, a q inside with ids[q] != k counts in column other[q]; the last index is the axis of the shared
 * face.  A value of other[q] at or above num_other counts nowhere.  other may be `ids` itself (class mode). */
int ru3d_label_faces(const void* ids, int id_bytes, const uint8_t* other, int num_other, int X, int Y, int Z, int count,
                     int64_t* table, void* stream);
/* extents: frames (device float64 [count][3][4]) holds three rows (ax, ay, az, b) per id; out (float64 [count][3][2]) =
 * the minimum and the maximum of t = ax x + ay y + az z + b over the id's voxels, (+inf, -inf) for an id without one. */
int ru3d_label_extents(const void* ids, int id_bytes, int X, int Y, int Z, int count, const double* frames, double* out,
                       void* stream);
/* The longest centre-to-centre distance inside each id under the metric d^2 = D^T G D.  Candidates are the first and the
 * last voxel of the id in every (x, y) row along Z: no other voxel is an extreme point of the id's voxel set.
 * count: counts (int64 [count]) = candidates per id.
 * fill: starts (int64 [count]) = where each id's group begins in `candidates` (int32 [capacity], linear voxel indices;
 * the exclusive prefix sums of counts, made by the caller); filled (int64 [count]) leaves equal to counts.  Inside a
 * group the order is not defined; nothing is written at or beyond `capacity`, and only the groups are written.
 * feret: total = the filled prefix of `candidates`; gram: HOST float64 [6] = G00, G11, G22, G01, G02, G12.  row_d2
 * (float64 [total]) and row_partner (int32 [total]) receive, per candidate, its largest squared distance to a candidate
 * of its id and the linear index that reaches it.  out_d2 (float64 [count]) = the largest of them, out_pair (int32
 * [count][6]) = (x, y, z) of its two voxels; ties go to the smallest pair of linear indices.  An id of one voxel gives 0
 * and the voxel twice, an id without a voxel -1 and six times -1. */
int ru3d_label_feret_count(const void* ids, int id_bytes, int X, int Y, int Z, int count, int64_t* counts, void* stream);
int ru3d_label_feret_fill(const void* ids, int id_bytes, int X, int Y, int Z, int count, const int64_t* starts,
                          int64_t* filled, int32_t* candidates, int64_t capacity, void* stream);
int ru3d_label_feret(const void* ids, int id_bytes, int X, int Y, int Z, int count, const int32_t* candidates,
                     int64_t total, const int64_t* starts, const int64_t* counts, const double* gram, double* row_d2,
                     int32_t* row_partner, double* out_d2, int32_t* out_pair, void* stream);

/* ------------------------------------------------------------------ binary morphology on packed masks + confusion table */
/* The clean-up and the evaluation of a prediction (nb_post.py:88-112, nb.py:11-37) on volumes that stay in HBM.
 * A packed mask holds 64 voxels of the contiguous Z axis per 64-bit word: bit b of word w of row (x, y) is voxel
 * z = 64 w + b; a row has ceil(Z / 64) words and the rows follow each other in the volume's [X, Y] order
 * (ru3d_mask_bytes = X * Y * ceil(Z / 64) * 8).  Every packed volume these calls write has zeros in the bits at
 * z >= Z of a row's last word.  X*Y*Z must stay below 2^31.  Nothing here needs a workspace. */
enum { RU3D_MASK_NE = 0, RU3D_MASK_EQ = 1, RU3D_MASK_GT = 2, RU3D_MASK_GE = 3 };
enum { RU3D_MORPH_ERODE = 0, RU3D_MORPH_DILATE = 1 };
#define RU3D_MORPH_MAX_EXTENT 15 /* odd extents up to 15 per axis: offsets -7 .. 7 */
#define RU3D_MORPH_MAX_ROWS 225
/* one (dx, dy) row of a structuring element: bit k of zmask stands for the offset (dx, dy, k - 7) */
typedef struct ru3d_morph_row {
    int8_t dx, dy;
    uint16_t zmask;
} ru3d_morph_row;
size_t ru3d_mask_bytes(int X, int Y, int Z);
/* bits = (src != 0), (src == value), (src > value) or (src >= value) of a uint8 [X, Y, Z] volume (`value` is ignored
 * by RU3D_MASK_NE): `pred == 2` or `pred > 0` without a byte mask in between. */
int ru3d_mask_pack(const uint8_t* src, int X, int Y, int Z, int op, int value, uint64_t* bits, void* stream);
/* paint == 0: dst = bit ? value : 0 over the whole uint8 [X, Y, Z] volume; paint == 1: dst = value where the bit is
 * set, untouched elsewhere (`output[mask] = value`). */
int ru3d_mask_unpack(const uint64_t* bits, int X, int Y, int Z, int value, int paint, uint8_t* dst, void* stream);
/* One erosion (dst[p] = AND over the offsets o of src[p + o]) or dilation (OR) of a packed volume, not in place;
 * voxels outside the volume read as border_value (0 or 1).  `rows` is a HOST array of num_rows (1 .. 225) rows with
 * |dx|, |dy| <= 7 and a non-empty zmask; it travels in the kernel arguments, nothing is uploaded.  The offsets are
 * gathered as given: scipy.ndimage.binary_erosion by a centred structure S is the offsets {s - centre}, and
 * binary_dilation is the reflected set {centre - s}. */
int ru3d_binary_morph(const uint64_t* src, uint64_t* dst, int X, int Y, int Z, int op, const ru3d_morph_row* rows,
                      int num_rows, int border_value, void* stream);
/* scipy.ndimage.binary_propagation on packed volumes (csrc/propagate.hip).  `reach` holds the seed on entry and is
 * grown in place: a voxel of `allowed` (of its complement inside the volume with invert_allowed = 1) is set once one of
 * its neighbours is - the 6 face neighbours for connectivity 1, all 26 for connectivity 3.  A seed voxel outside
 * `allowed` stays set and spreads like any other, as in scipy.  A voxel outside the volume reads as set when every
 * axis along which it is outside (0 = X, 1 = Y, 2 = Z) has its bit in border_axes, else as clear; a volume of fewer
 * axes names only the axes it has.  The call clears changed_dev[0 .. rounds) (device int32, 1 <= rounds <= 64) and
 * runs `rounds` rounds as `rounds` launches; changed_dev[r] = the tiles that grew in round r.  A round that counts 0 is
 * the fixpoint, and later rounds only read.  Convergence is the caller's loop: download the counters, stop when the
 * last is 0, else call again.  The fixpoint is unique, so the result is the same bytes in every run.  `allowed` is
 * only read and may carry set bits at z >= Z; `reach` must not. */
int ru3d_binary_propagate(const uint64_t* allowed, int invert_allowed, uint64_t* reach, int X, int Y, int Z,
                          int connectivity, int border_axes, int rounds, int32_t* changed_dev, void* stream);
/* out = mask | ~reach inside the volume (binary_fill_holes: reach = what the outside floods of the complement of mask),
 * zeros at z >= Z; three buffers, not in place. */
int ru3d_mask_fill_result(const uint64_t* mask, const uint64_t* reach, uint64_t* out, int X, int Y, int Z, void* stream);
/* table (device int64 [(C + 1)][(C + 1)], C = num_classes <= 32; zeroed by the call, on `stream`):
 * table[min(label[i], C)][min(pred[i], C)] += 1 over n < 2^31 voxels of two uint8 volumes of any alignment.  Integer
 * atomics only: exact, and the same in every run.  The grid is sized by ru3d_get_cu_budget(). */
int ru3d_confusion_counts(const uint8_t* pred, const uint8_t* label, int64_t n, int num_classes, int64_t* table,
                          void* stream);

/* ------------------------------------------------------------------ dataset preparation */
/* What orient_crop_case / analyze_cases (reference data.py:117-172, 322-461) need beyond data movement, for a case that
 * lives in HBM.  `image` is the case layout, fp32 [X, Y, Z, C] dense with the channel last; fewer than 2^31 voxels.
 * Every result is exact and the same in every run: integer atomics and fixed-order sums only.
 *
 * ru3d_threshold_bbox: box (device int32 [6]) = per axis the smallest and the LARGEST index (x0, x1, y0, y1, z0, z1) of a
 * voxel with any channel > threshold, count (device int64) = the number of such voxels.  count == 0 leaves the box at
 * (INT_MAX, -1) per axis.  One read of the volume. */
int ru3d_threshold_bbox(const float* image, int X, int Y, int Z, int C, float threshold, int32_t* box, int64_t* count,
                        void* stream);
/* ru3d_masked_sample: out = image[..., channel][label > 0][::stride] in numpy's element order (x outermost, z fastest):
 * the foreground voxel of rank r goes to out[r / stride] when r % stride == 0.  `label` is uint8 or int64 [X, Y, Z]
 * (RU3D_LABEL_U8 / RU3D_LABEL_I64).  count (device int64) receives the number of samples, ceil(foreground / stride),
 * whatever the capacity; nothing is written at or beyond out[capacity], so a count above the capacity means the buffer
 * was too small.  out == NULL counts only (image may then be NULL as well).  Workspace: one int per 2048 voxels. */
size_t ru3d_masked_sample_workspace_bytes(int X, int Y, int Z);
int ru3d_masked_sample(const float* image, int X, int Y, int Z, int C, int channel, const void* label, int label_dtype,
                       int stride, float* out, int64_t capacity, int64_t* count, void* ws, size_t ws_bytes, void* stream);
/* ru3d_order_stats: out[i] (device fp32) = the ranks[i]-th smallest of n finite device values, zero-based - the value
 * np.sort(values)[ranks[i]] (the two zeros are one value: compare with ==).  `ranks` is a HOST array of 1 ..
 * RU3D_ORDER_STATS_MAX_RANKS entries, each < n.  Radix select, 8 bits per pass: the values are read four times, never
 * moved. */
#define RU3D_ORDER_STATS_MAX_RANKS 8
size_t ru3d_order_stats_workspace_bytes(void);
int ru3d_order_stats(const float* values, int64_t n, const int64_t* ranks, int num_ranks, float* out, void* ws,
                     size_t ws_bytes, void* stream);
/* ru3d_moments: out (device float64 [5]) = (n, min, max, mean, population standard deviation) of n finite device
 * values, accumulated in float64 in two passes (sum; squared deviations from the mean). */
size_t ru3d_moments_workspace_bytes(void);
int ru3d_moments(const float* values, int64_t n, double* out, void* ws, size_t ws_bytes, void* stream);

/* ------------------------------------------------------------------ distance transform + surface-distance reductions */
/* Boundary metrics of a prediction that stays in HBM (Hausdorff distance, its percentile, average symmetric surface
 * distance, surface Dice).  Masks are the packed masks of the morphology section; X*Y*Z < 2^31.
 *
 * ru3d_edt_squared: the exact squared Euclidean distance transform.  The set bits of `bits` are the FEATURE voxels,
 * `spacing` is a HOST array of three finite values > 0, out is float64 [X, Y, Z]:
 *     out[p] = min over the feature voxels f of  fl(A + fl(B + C)),
 *     A = fl(fl(sx (px - fx))^2),  B = fl(fl(sy (py - fy))^2),  C = fl(fl(sz (pz - fz))^2)
 * in float64, fl = round to nearest.  That expression is the contract: the result does not depend on the order the
 * candidates are visited in and can be compared with ==.  No feature voxel at all: +inf everywhere.  X and Y may not
 * exceed RU3D_EDT_MAX_AXIS (a column of the scanned axis is held in LDS); Z is bounded by the voxel count alone. */
#define RU3D_EDT_MAX_AXIS 4096
size_t ru3d_edt_workspace_bytes(int X, int Y, int Z);
int ru3d_edt_squared(const uint64_t* bits, int X, int Y, int Z, const double* spacing, double* out, void* ws,
                     size_t ws_bytes, void* stream);
/* dst = src & ~erode(src) with the 6-neighbour cross and border_value 0, not in place: the voxels of the mask that have
 * a face neighbour outside it, the volume's faces counting as outside. */
int ru3d_mask_surface(const uint64_t* src, uint64_t* dst, int X, int Y, int Z, void* stream);
/* values[r] = sq[p_r] for the set bits p_r of `query` in numpy's element order (x outermost, z fastest): numpy's
 * sq[query].  count (device int64) receives the number of set bits whatever the capacity; nothing is written at or
 * beyond values[capacity].  values == NULL counts only (sq may then be NULL as well).  Workspace: one int per 256
 * words of the mask. */
size_t ru3d_edt_gather_workspace_bytes(int X, int Y, int Z);
int ru3d_edt_gather(const double* sq, const uint64_t* query, int X, int Y, int Z, double* values, int64_t capacity,
                    int64_t* count, void* ws, size_t ws_bytes, void* stream);
/* out (device float64 [4]) = (n, max v, #{v <= tau_sq}, sum of sqrt(v)) over the first n = min(*count, capacity)
 * device values v >= 0; `count` is a DEVICE int64, so a gather and its reductions are enqueued without a host read in
 * between.  n == 0 gives four zeros.  The sum runs in float64 over a fixed partition in a fixed order: the same bits
 * in every run and under every CU budget.  The square root is monotone, so maximum and count are taken on the squared
 * distances and are exact. */
size_t ru3d_edt_reduce_workspace_bytes(int64_t capacity);
int ru3d_edt_reduce(const double* values, const int64_t* count, int64_t capacity, double tau_sq, double* out, void* ws,
                    size_t ws_bytes, void* stream);

/* ------------------------------------------------------------------ skeleton */
/* Curve skeletons of tubular structures (vessels) and what is measured on them: centreline Dice, end and branch
 * voxels, centreline length, radii.  Masks are the packed masks of the morphology section; X*Y*Z < 2^31.
 *
 * The thinning.  Objects are 26-connected, the background is 6-connected, voxels outside the volume are background.
 * N26*(p) is the 26 neighbours of p without p.
 *   Simple voxel.  An object voxel p such that (T26 = 1) the object voxels of N26*(p) are not empty and form exactly one
 *                  26-connected component, and (T6bar = 1) the background voxels of the 18-neighbourhood of p include a
 *                  6-neighbour of p and all background 6-neighbours of p lie in one 6-connected component of that
 *                  18-neighbourhood background.  An interior voxel and an isolated voxel are not simple.
 *   End voxel.     An object voxel with exactly one object voxel in N26*(p).  End voxels are kept: a curve skeleton.
 *   Iteration.     For each direction d in the order -x, +x, -y, +y, -z, +z: (1) the candidates are the object voxels
 *                  whose neighbour at p + d is background, on the mask as it is when the direction begins; (2) for each
 *                  subfield s = 4 (x & 1) + 2 (y & 1) + (z & 1) in the order 0 .. 7, every candidate of subfield s
 *                  that is simple and not an end voxel is deleted, both predicates evaluated on the mask as it is when
 *                  that sub-pass begins.  No two voxels of a subfield are 26-adjacent, so the deletions of a sub-pass
 *                  cannot influence one another: the result does not depend on thread order or launch geometry.
 *   Iterations repeat until one whole iteration deletes nothing (that last iteration is counted), or max_iterations.
 *
 * ru3d_skeleton_thin thins `mask` in place on `stream`, reads the deletion counter back once per iteration and
 * returns the number of iterations run (>= 0), or a negative status.  max_iterations < 0: until nothing changes.
 * Workspace: the candidate mask and the counters. */
size_t ru3d_skeleton_workspace_bytes(int X, int Y, int Z);
int ru3d_skeleton_thin(uint64_t* mask, int X, int Y, int Z, int max_iterations, void* ws, size_t ws_bytes, void* stream);
/* ends / junctions (packed, distinct from skel and from each other) = the set voxels with exactly 1 / with 3 or more
 * set voxels among their 26 neighbours; counts (device int64 [3]) = (set voxels, end voxels, junction voxels). */
int ru3d_skeleton_classify(const uint64_t* skel, int X, int Y, int Z, uint64_t* ends, uint64_t* junctions, int64_t* counts,
                           void* stream);
/* out (device float64 [1]) = the length of the voxel graph: over the 13 offsets o = (dx, dy, dz) of cells 14 .. 26 of
 * the 3 x 3 x 3 cube (index 9 (dx + 1) + 3 (dy + 1) + (dz + 1); each unordered pair of 26-adjacent voxels once), in
 * that order, total = fl(total + fl(pairs(o) * step(o))) with pairs(o) the number of set voxels p with p + o set and
 * step(o) = sqrt(fl(A + fl(B + C))), A = fl(fl(sx dx)^2), in float64.  `spacing` is a HOST array of three finite
 * values > 0.  Every edge of the graph counts, so the short diagonals inside the clique of voxels at a junction are
 * included: on a curve without junctions this is the curve's length, at each branch point it adds a few voxel steps.
 * Workspace: 256 bytes. */
int ru3d_skeleton_length(const uint64_t* skel, int X, int Y, int Z, const double* spacing, double* out, void* ws,
                         size_t ws_bytes, void* stream);
/* counts (device int64 [3]) = (|a|, |b|, |a & b|) of two packed masks of one shape: with a skeleton and a mask, the
 * integers centreline Dice is made of. */
int ru3d_skeleton_overlap(const uint64_t* a, const uint64_t* b, int X, int Y, int Z, int64_t* counts, void* stream);
/* out (device float64 [4]) = (n, min v, max v, sum of sqrt(v)) over n device values v >= 0 (squared radii gathered at
 * the skeleton voxels); n == 0 gives (0, +inf, 0, 0).  The sum has a fixed order: 256 partial sums, partial t over the
 * elements t, t + 256, .. in order starting from 0, then seven halving steps s[t] = fl(s[t] + s[t + h]), h = 128 .. 1. */
int ru3d_skeleton_radius_stats(const double* sq, int64_t n, double* out, void* stream);

/* ------------------------------------------------------------------ skeleton graph */
/* The voxel graph of a packed mask S as nodes and branches: how many segments a vessel tree has, which segment hangs on
 * which branch point, how long and how thick each one is.  S is any packed mask, thin or not, X*Y*Z < 2^31; bits at
 * z >= Z are ignored.  Adjacency is the 26-neighbourhood, deg(p) the number of set voxels in N26*(p).  Every order
 * below is element order (x slowest, z fastest), a linear index is (x Y + y) Z + z.
 *
 *   Voxel kinds.  A path voxel has deg(p) == 2; every other set voxel (deg 0, 1 or >= 3) is a node voxel.
 *   Nodes.        The 26-connected components of the node voxels.  An end voxel that touches a junction clique belongs
 *                 to that node (a one-voxel spur is absorbed); two node voxels that touch are never two nodes.
 *   Branches.     The 26-connected components of the path voxels.  Each of a path voxel's two neighbours is a path voxel
 *                 of the same branch or a node voxel, so a branch is a simple path with exactly two attachments to nodes
 *                 (possibly to the same node; a path of one voxel attaches with both its neighbours) or a closed loop
 *                 with none.  Every edge of the voxel graph lies in exactly one branch or inside exactly one node.
 *   Numbering.    Nodes 1 .. M and branches 1 .. B, each in the order of their first voxel (ru3d_label_components).
 *   ids           int32, one per set voxel in element order (the order of ru3d_edt_gather): +b on a voxel of branch b,
 *                 -m on a voxel of node m.
 *   nodes         int64 [M, 6]: voxels, valence (the number of attachments; a branch attached twice counts twice),
 *                 sum_x, sum_y, sum_z (integer coordinate sums), first (the linear index of its first voxel).
 *   branches      int64 [B, 18]: voxels; t0, t1, the linear indices of the two terminal path voxels, t0 <= t1; n0, n1,
 *                 the nodes attached at t0 and at t1, n0 <= n1 when t0 == t1 (all four -1 for a loop); pairs[13], per
 *                 offset o of cells 14 .. 26 (the indexing of ru3d_skeleton_length) the unordered pairs {p, q} of
 *                 adjacent set voxels that differ by +-o with at least one of them a path voxel of this branch, each
 *                 pair once, the attachment edges included.  A length is not computed here: a caller folds pairs with
 *                 the expression of ru3d_skeleton_length and gets the numpy route's bits.
 *   branch_radii  [B, 3] of 8 bytes, with sq (float64 [X, Y, Z], squared radii >= 0, radius < 2^15 units): float64
 *                 rmin_sq and rmax_sq, exact over the branch's path voxels, and int64 rsum_q = the sum over its path
 *                 voxels with finite v of llrint(sqrt(v) 2^24) - the square root is correctly rounded and the scaling
 *                 exact, so this is an integer sum without an order.  +inf shows in rmax_sq and adds nothing to the sum.
 * Integer atomics only: the same bytes in every run and under every CU budget.
 *
 * ru3d_skeleton_graph_label: counts (device int64 [3]) = (set voxels n, M, B); nothing is written at or beyond
 * ids[capacity].  When n > capacity nothing is labelled, ids is left alone and M = B = 0: the caller compares
 * counts[0] with its capacity.  ids == NULL with capacity == 0 counts the voxels only.  No host read.
 * ru3d_skeleton_graph_measure fills the tables from the ids of the same mask (n, M, B: what label counted); sq and
 * branch_radii are both given or both NULL.  ru3d_skeleton_graph_erase clears, in place, the voxels of the branches b
 * with flags_branch[b - 1] != 0 and of the nodes m with flags_node[m - 1] != 0 (device bytes [B] and [M]).
 * Workspace, all three: 3 * ru3d_skeleton_workspace_bytes(X, Y, Z) - the prefix sums of the ranks, the path voxels and
 * the first voxels of the nodes and branches, a 64-bit plane of the packed words or less each. */
int ru3d_skeleton_graph_label(const uint64_t* skel, int X, int Y, int Z, int32_t* ids, int64_t capacity, int64_t* counts,
                              void* ws, size_t ws_bytes, void* stream);
int ru3d_skeleton_graph_measure(const uint64_t* skel, int X, int Y, int Z, const int32_t* ids, int64_t n, int64_t M, int64_t B,
                                const double* sq, int64_t* nodes, int64_t* branches, void* branch_radii, void* ws,
                                size_t ws_bytes, void* stream);
int ru3d_skeleton_graph_erase(uint64_t* skel, int X, int Y, int Z, const int32_t* ids, int64_t n, int64_t M, int64_t B,
                              const uint8_t* flags_branch, const uint8_t* flags_node, void* ws, size_t ws_bytes, void* stream);

/* ------------------------------------------------------------------ nearest site / territories */
/* Which set voxel of a packed mask (a SITE: a centreline voxel of a vessel tree) is nearest to every voxel, the labels
 * of a region by nearest site (a Voronoi partition: the territory of every branch) and their integer tally against a
 * second label volume.  Masks are the packed masks of the morphology section, X*Y*Z < 2^31, a linear index is
 * (x Y + y) Z + z, element order is the order of the linear index.
 *
 * ru3d_nearest_site: the exact Euclidean feature transform.  `spacing` is a HOST array of three finite values > 0 whose
 * squared steps neither overflow nor underflow.  index (int32 [X, Y, Z]) receives the linear index of the nearest set
 * voxel of `bits`, sq (float64 [X, Y, Z], or NULL) the squared distance to it, with exactly the bits ru3d_edt_squared
 * gives for the same mask and spacing.  The site is chosen separably and BY VALUE, fl = round to nearest in float64:
 *   Z pass   among the set voxels (x, y, z') of the voxel's own column the one with the least C = fl(fl(sz (z - z'))^2),
 *            the smaller z' on equal C;  C_best(x, y, z) is that value, +inf for a column without a set voxel;
 *   Y pass   over y' the least fl(B + C_best(x, y', z)), B = fl(fl(sy (y - y'))^2), the smaller y' on equal value;
 *   X pass   over x' the least fl(A + (the Y pass's value at (x', y, z))), the smaller x' on equal value;
 * and the site is the one the chosen (x', y', z') chain ends in.  Rounding is monotone, so the value equals the minimum
 * over all sites of fl(A + fl(B + C)); with a spacing whose products are exact (unit, dyadic) the site is the one of
 * least squared distance and, among those, of smallest linear index.  No set voxel at all: index -1 and sq +inf
 * everywhere.  X and Y may not exceed RU3D_EDT_MAX_AXIS.  Workspace: ru3d_edt_workspace_bytes(X, Y, Z), and with
 * sq == NULL 8 X Y Z bytes more (the values have to live somewhere between the passes). */
int ru3d_nearest_site(const uint64_t* bits, int X, int Y, int Z, const double* spacing, int32_t* index, double* sq, void* ws,
                      size_t ws_bytes, void* stream);
/* labels (int32 [X, Y, Z]) = site_ids[rank(index[p])] where the bit of region_bits is set (everywhere with NULL) and
 * index[p] >= 0, and 0 everywhere else.  rank(f) is the position of voxel f among the set bits of site_bits in element
 * order - the order of ru3d_edt_gather and of the ids of ru3d_skeleton_graph_label - and site_ids is a device int32 [n].
 * Checked on the device, nothing out of bounds read or written: n must be the number of set bits of site_bits (else
 * every label is 0) and every index >= 0 inside the region a set voxel of site_bits (else that label is 0); either
 * returns -2.  The call reads one word back: it returns after its kernels have run.  Workspace:
 * 2 * ru3d_skeleton_workspace_bytes(X, Y, Z) - the error word, one int per 256 words of the mask and one int per word. */
int ru3d_site_assign(const uint64_t* site_bits, const uint64_t* region_bits, const int32_t* index, const int32_t* site_ids,
                     int64_t n, int X, int Y, int Z, int32_t* labels, void* ws, size_t ws_bytes, void* stream);
/* table (int64 [K + 1, num_other + 1], overwritten) [labels[p]] [min(other[p], num_other)] += 1 over the voxels of
 * region_bits (all voxels with NULL); `other` is a uint8 volume or NULL with num_other == 0 (one column).  Row 0 holds
 * the region's voxels without a site.  A label outside 0 .. K is not counted and returns -2.  Integer counts only: the
 * same table in every run and under every CU budget.  The call reads one word back, as ru3d_site_assign does.
 * Workspace: 256 bytes. */
int ru3d_territory_tally(const int32_t* labels, int K, const uint8_t* other, int num_other, const uint64_t* region_bits,
                         int X, int Y, int Z, int64_t* table, void* ws, size_t ws_bytes, void* stream);

/* ------------------------------------------------------------------ geodesic distance */
/* What is nearest along a path that stays inside a mask, and how long that path is (csrc/geodesic.hip): a multi-source
 * shortest-path transform on the 6- or 26-neighbour voxel graph of a packed mask, the weighted version of
 * ru3d_binary_propagate.  Volumes are [X, Y, Z] with X*Y*Z < 2^31, masks the packed masks of the morphology section.
 *
 * Operands.  seeds (int32 volume): 0 = no seed, > 0 = the seed's label, < 0 raises flags_dev[0].  allowed: a packed mask
 * (its complement inside the volume with invert_allowed = 1), NULL = every voxel; it is only read and may carry set
 * bits at z >= Z.
 * Step lengths are integers.  weights is a HOST array of 26 uint32, one per offset d in {-1, 0, 1}^3 without the centre
 * in ascending (dx, dy, dz); 0 = no such step, else 1 .. 2^20.  The caller forms them, for a spacing s and a quantum q,
 * as w(d) = rint(sqrt(sum (d_i s_i)^2) / q) in float64, half to even (geodesic.step_weights).  Only face steps non-zero
 * is connectivity 1, all 26 connectivity 3; any other pattern runs as given.
 * State is one 64-bit key per voxel: key = dist << 32 | label, all ones = not reached.  ru3d_geodesic_init writes
 * key = label (distance 0) at a seed, whether or not it lies in `allowed` - as in ru3d_binary_propagate a seed outside
 * `allowed` stays and spreads into its allowed neighbours - and all ones elsewhere.
 * Relaxation rule.  For a voxel v of `allowed` and its neighbour u = v + d with a reached key, w the weight of d:
 *   key[v] = min(key[v], key[u] + (w << 32)),   admitted only when dist(u) + w <= limit.
 * limit is the caller's bound in quanta, at most 0xFFFFFFFE; 0xFFFFFFFE itself stands for "no bound".
 * The result is the least fixpoint of the rule.  Integer addition makes (dist, label) strictly monotone under a step,
 * so it equals a lexicographic Dijkstra: per voxel the smallest distance and, among the seeds at that distance, the
 * smallest label.  It is unique: the same bytes in every run, whatever the order of updates and however stale a read.
 * Overflow.  With limit == 0xFFFFFFFE a round raises flags_dev[1] when it leaves an allowed voxel unreached although
 * a reached neighbour's step to it was turned down.  While the rounds run that can be a passing state; at the fixpoint
 * it says that a distance does not fit 32 bits (use a larger quantum).  So the caller confirms a raised flag: clear it,
 * run one round on the converged keys with first = 1 (every tile looks) and read it again.  A limit below 0xFFFFFFFE
 * never raises it.
 *
 * ru3d_geodesic_init clears flags_dev[0 .. 2) (device int32) and the workspace's activity maps and writes the keys.
 * ru3d_geodesic_rounds clears changed_dev[0 .. rounds) (device int32, 1 <= rounds <= 64) and runs `rounds` rounds as
 * `rounds` launches on tiles of 8 x 8 x 32 voxels; changed_dev[r] = the tiles that stored a key in round r.  A tile
 * relaxes its voxels from LDS until nothing falls or RU3D_GEODESIC_MAX_TRIPS trips are done and stores the keys that
 * fell.  A round that counts 0 is the fixpoint and later rounds only read.  Convergence is the caller's loop, as for
 * ru3d_binary_propagate.  The workspace holds two byte maps of tile activity: with skip_idle = 1 a tile whose own and
 * 26 neighbouring tiles stored nothing in the round before exits at once - that round may be the last one of the call
 * before on the same keys and workspace; first = 1 says there is none and makes every tile of round 0 run.
 * skip_idle = 0 runs every tile in every round; the keys are the same bytes either way.
 * ru3d_geodesic_split: dist (uint32) = the key's high half, 0xFFFFFFFF where not reached; labels (int32) = its low
 * half, 0 where not reached.  Distances in the spacing's unit are dist * q.
 * Workspace (init and rounds, the same buffer): ru3d_geodesic_workspace_bytes(X, Y, Z). */
#define RU3D_GEODESIC_MAX_TRIPS 32 /* relaxation trips of a tile inside one round */
size_t ru3d_geodesic_workspace_bytes(int X, int Y, int Z);
int ru3d_geodesic_init(const int32_t* seeds, uint64_t* keys, int X, int Y, int Z, int32_t* flags_dev, void* ws,
                       size_t ws_bytes, void* stream);
int ru3d_geodesic_rounds(const uint64_t* allowed, int invert_allowed, uint64_t* keys, int X, int Y, int Z,
                         const uint32_t* weights, uint32_t limit, int rounds, int first, int skip_idle, int32_t* changed_dev,
                         int32_t* flags_dev, void* ws, size_t ws_bytes, void* stream);
int ru3d_geodesic_split(const uint64_t* keys, uint32_t* dist, int32_t* labels, int X, int Y, int Z, void* stream);

/* ------------------------------------------------------------------ local thickness */
/* How thick a structure is at each of its voxels (csrc/thickness.hip): the squared radius of the largest inscribed ball
 * that contains the voxel (Hildebrand and Rueegsegger 1997) - vessel calibre at every lumen voxel, parenchymal and wall
 * thickness.  Volumes are [X, Y, Z] with X*Y*Z < 2^31, a linear index is (x Y + y) Z + z, masks are the packed masks of
 * the morphology section.  M is the set of set bits of the mask, s the spacing (a HOST array of three finite values
 * > 0).  All arithmetic is float64, fl = round to nearest, no contraction:
 *     d2(x, p) = fl(A + fl(B + C)),  A = fl(fl(sx (xx - px))^2),  B and C alike for y and z
 *                (the expression of ru3d_edt_squared),
 *     R2(p)    = min over the CLEAR voxels b inside the volume of d2(p, b), for p in M: the bits ru3d_edt_squared gives
 *                for the complement of the mask.  The volume's faces are not background (scipy's convention, the EDT's),
 *     T2(x)    = max { R2(p) : p in M, d2(x, p) < R2(p) } for x in M, with strict <;  T2(x) = 0 for x outside M.
 * No clear voxel in the volume: T2 = +inf on every voxel.  Empty mask: T2 = 0 everywhere.  The thickness is
 * 2 sqrt(T2) in the unit of the spacing.  This is a formula, not an algorithm: results compare with ==, and a maximum
 * does not depend on the order of its operands, so the bytes are the same in every run.
 * Consequences:
 *   - p = x always qualifies (d2 = 0 < R2), so T2 >= R2 on M;
 *   - every value of T2 on M is a value of R2;
 *   - with strict < a ball never contains a clear voxel b (d2(b, p) = d2(p, b) >= R2(p)), so painting the balls needs
 *     no test of the mask;
 *   - distances run between voxel CENTRES: a slab of k voxels reads k voxels thick for even k and k + 1 for odd k
 *     (its middle voxel is (k + 1) / 2 steps from the nearest clear voxel on both sides).  This is the definition on
 *     a grid and is not corrected for.
 *
 * ru3d_thickness_candidates: index[r] (int32) = the linear index of the r-th set bit of `bits` in element order (the
 * order of ru3d_edt_gather); count (device int64) receives the number of set bits whatever the capacity; nothing is
 * written at or beyond index[capacity].  index == NULL counts only.  `bits` is only read and may carry set bits at
 * z >= Z.  Workspace: ru3d_thickness_workspace_bytes(X, Y, Z) - one int per 256 words of the mask -, aligned to 8 bytes;
 * a short or misaligned one is refused before any launch.
 * ru3d_thickness_paint: out (float64 [X, Y, Z], overwritten, not r2) = T2 from the n candidates index[0 .. n) (device
 * int32) and the float64 volume r2 of their squared radii, R2(p) = r2[index[i]]: out is cleared, and every candidate
 * paints R2(p) by maximum into the voxels x of its bounding box with d2(x, p) < R2(p).  A candidate with
 * R2 == +inf stores +inf at its own voxel alone (with no clear voxel every voxel is a candidate); one with R2 <= 0
 * or an index outside the volume paints nothing.  The order of the list changes the work, never the bytes: painting the
 * large balls first lets most later tests end at a plain load.  work_dev: NULL, or a device int64 [2] that receives the
 * voxels tested against the contract's expression and the atomic updates issued.
 *
 * The three prototypes stand in ru3d_since.h, included here: the prototypes of this file are held one to one against
 * _native.SIGNATURES, and entry points added since the tests' case table was last brought up to date are bound from
 * _native.SIGNATURES_SINCE; the two are folded back together. */
#include "ru3d_since.h"

/* ------------------------------------------------------------------ soft skeletons, soft-clDice loss */
/* The soft skeleton of Shit et al. (clDice, CVPR 2021) on float32 volumes x[A][B][Z] (Z fastest), `nvol` of them behind
 * one another; nothing outside a volume takes part and nothing crosses from one volume into the next.
 *   E(x)[v] = min over v and its face neighbours inside the volume; D(x)[v] = max over the 3x3x3 block inside the volume;
 *   x_0 = x, x_{j+1} = E(x_j), d_j = relu(x_j - D(x_{j+1})), s_0 = d_0, s_j = s_{j-1} + relu(d_j - s_{j-1} d_j), j <= k.
 *   relu' is 0 at 0.  A minimum / maximum hands its gradient to ONE voxel of its window: among equal candidates the one
 *   with the lowest linear index (a B + b) Z + z.  Candidate order of E: (a-1), (b-1), (z-1), centre, (z+1), (b+1), (a+1);
 *   of D: the 27 offsets in ascending (da, db, dz).
 * A "plane" is nvol * A * B * Z elements.  The forward fills, for j = 0 .. k (k = iterations, 0 .. 64), plane j of
 *   delta (float32: d_j), s (float32: s_j; the result is plane k), emin (uint8: which candidate of E gave x_{j+1}) and
 *   dmax (uint8: which candidate of D was taken for d_j); the backward reads exactly these, never x.
 * Everything is stream-ordered, allocates nothing, takes no atomics (two runs give the same bits) and may be captured.
 * Workspace for both directions and for the loss: ru3d_cldice_workspace_bytes(nvol, ...), nvol = N * selected classes. */
size_t ru3d_cldice_workspace_bytes(int nvol, int A, int B, int Z, int iterations);
int ru3d_soft_skeleton_fwd(const float* x, int nvol, int A, int B, int Z, int iterations, float* delta, float* s,
                           uint8_t* emin, uint8_t* dmax, void* ws, size_t ws_bytes, void* stream);
/* grad_x (one plane, distinct from the workspace) = d<grad_out, s_k>/dx. */
int ru3d_soft_skeleton_bwd(const float* grad_out, int nvol, int A, int B, int Z, int iterations, const float* delta,
                           const float* s, const uint8_t* emin, const uint8_t* dmax, float* grad_x, void* ws,
                           size_t ws_bytes, void* stream);
/* Soft-clDice loss.  P = softmax(logits) in float32 (logits addressed as in ru3d_loss_fwd, C = num_classes >= 2),
 * G = one-hot(labels); `classes` (HOST array of num_selected distinct class numbers) selects the volumes (n, class);
 *   Tprec_c = (sum S_k(P_c) G_c + eps) / (sum S_k(P_c) + eps), Tsens_c = (sum S_k(G_c) P_c + eps) / (sum S_k(G_c) + eps),
 *   loss = sum_c w_c (1 - 2 Tprec_c Tsens_c / (Tprec_c + Tsens_c)), sums over the batch's samples and voxels jointly,
 *   w = weight_v (HOST array of C floats, NULL: ones) restricted to `classes` over the sum of its absolute values.
 * delta, s, emin, dmax: as above for nvol = n * num_selected, volume (n, slot) at index n * num_selected + slot;
 * skel_g: one float32 plane, receives S_k(G) (no gradient flows through it).  state: ru3d_cldice_state_bytes() bytes;
 * the count of labels outside [0, C) sits at ru3d_loss_state_bad_labels_offset() as in the fused losses' state (the
 * loss is NaN then).  loss_out: 1 float32 on the device. */
size_t ru3d_cldice_state_bytes(void);
int ru3d_cldice_fwd(const float* logits, int64_t stride_n, int64_t stride_c, int64_t stride_v, const void* labels,
                    int label_dtype, int n, int A, int B, int Z, int num_classes, const int* classes, int num_selected,
                    int iterations, const float* weight_v, float smooth, float* delta, float* s, uint8_t* emin,
                    uint8_t* dmax, float* skel_g, void* state, float* loss_out, void* ws, size_t ws_bytes, void* stream);
/* dlogits (float32, the logits' strides) = or, with accumulate != 0, += grad_out[0] * scale * dloss/dlogits
 * (grad_out: device float32 or NULL for 1). */
int ru3d_cldice_bwd(const float* logits, int64_t stride_n, int64_t stride_c, int64_t stride_v, const void* labels,
                    int label_dtype, int n, int A, int B, int Z, int num_classes, const int* classes, int num_selected,
                    int iterations, const float* delta, const float* s, const uint8_t* emin, const uint8_t* dmax,
                    const float* skel_g, const void* state, const float* grad_out, float scale, int accumulate,
                    float* dlogits, void* ws, size_t ws_bytes, void* stream);

/* ------------------------------------------------------------------ signed distance maps, boundary loss */
/* The signed distance maps of a label patch labels[n][A][B][Z] (uint8 or int64 as in ru3d_loss_fwd, Z fastest), one per
 * sample and per selected class, all of them in ONE launch sequence whatever n and num_selected are.  `classes` is a
 * HOST array of num_selected distinct class numbers of [0, num_classes), 2 <= num_classes <= 8; volume (n, slot) lies at
 * index n * num_selected + slot of the outputs.  For sample n, class q = classes[slot], G = {u : labels[n][u] == q}:
 *   v outside G:  d2[v] = min over u in G     of |v - u|^2,  phi[v] = +sqrt(d2[v]),        d2_out[v] = +d2[v]
 *   v inside G:   d2[v] = min over u not in G of |v - u|^2,  phi[v] = -(sqrt(d2[v]) - 1),  d2_out[v] = -d2[v]
 *   (a foreground voxel on the boundary has phi = 0);
 *   G empty, or G the whole volume of that sample: phi = 0 and d2_out = 0 for that (n, slot) - no loss and no gradient
 *   from an absent class (Kervadec et al., MIDL 2019).  Decided on the device, per (n, slot), never by a host read.
 * Distances are in voxels: unit spacing on every axis, there is no `sampling` argument.  Nothing outside the patch exists
 * and the patch faces are not a boundary.  A label outside [0, num_classes) matches no class (it is background of every
 * selected class).  d2 is an exact integer, computed in int32; phi = float32(sqrt(d2)) correctly rounded and, inside,
 * the float32 difference to 1 negated.  No extent may exceed RU3D_BOUNDARY_MAX_AXIS (one column of a scanned axis is
 * held in LDS; 3 (L - 1)^2 stays below 2^24) and A*B*Z < 2^31: ru3d_boundary_workspace_bytes returns 0 and the entry
 * points an error status beyond that.  d2_out (int32) and phi_out (float32) hold nvol * A*B*Z elements, nvol =
 * n * num_selected; either may be NULL, not both.  Stream-ordered, allocates nothing, integer atomics only (two runs
 * give the same bits), may be captured. */
#define RU3D_BOUNDARY_MAX_AXIS 2048
size_t ru3d_boundary_workspace_bytes(int nvol, int A, int B, int Z);
int ru3d_signed_distance(const void* labels, int label_dtype, int n, int A, int B, int Z, int num_classes,
                         const int* classes, int num_selected, int32_t* d2_out, float* phi_out, void* ws,
                         size_t ws_bytes, void* stream);
/* Boundary loss.  P = softmax(logits) in float32 (logits addressed as in ru3d_loss_fwd, C = num_classes >= 2):
 *   loss = sum_{q in classes} w_q / (n V) sum_n sum_v P_q[n][v] phi_q[n][v],  V = A*B*Z,
 *   w = weight_v (HOST array of C floats, NULL: ones) restricted to `classes` over the sum of its absolute values.
 * The forward makes the maps (as above) into phi - a caller-owned buffer of n * num_selected * V float32 - and the
 * backward reads them: nothing is transformed twice.  The sum is taken in float64 over a partition fixed by the shape
 * and a fixed tree: the same bits in every run and under every CU budget.  state: ru3d_boundary_state_bytes() bytes; the
 * count of labels outside [0, C) sits at ru3d_loss_state_bad_labels_offset() as in the fused losses' state (the loss is
 * NaN then).  loss_out: 1 float32 on the device.  Workspace: ru3d_boundary_workspace_bytes(n * num_selected, ...). */
size_t ru3d_boundary_state_bytes(void);
int ru3d_boundary_fwd(const float* logits, int64_t stride_n, int64_t stride_c, int64_t stride_v, const void* labels,
                      int label_dtype, int n, int A, int B, int Z, int num_classes, const int* classes, int num_selected,
                      const float* weight_v, float* phi, void* state, float* loss_out, void* ws, size_t ws_bytes,
                      void* stream);
/* dlogits_j[n][v] (float32, the logits' strides) = or, with accumulate != 0, +=
 *   grad_out[0] * scale / (n V) * P_j (w_j phi_j [j in classes] - sum_q w_q P_q phi_q)
 * (grad_out: device float32 or NULL for 1; phi and state as the forward left them). */
int ru3d_boundary_bwd(const float* logits, int64_t stride_n, int64_t stride_c, int64_t stride_v, int n, int A, int B,
                      int Z, int num_classes, const int* classes, int num_selected, const float* phi, const void* state,
                      const float* grad_out, float scale, int accumulate, float* dlogits, void* stream);

/* ------------------------------------------------------------------ deep supervision */
/* The fused loss of ru3d_loss_fwd (kinds HYBIRD, DICELOSS, FOCAL; same formulas, precisions and scalars) on up to
 * RU3D_DS_MAX_LEVELS logits tensors of falling resolution at once, against ONE label tensor labels[n][D][H][W] (uint8 or
 * int64, contiguous): voxel (a, b, c) of a level with shift s has the label labels[a << s][b << s][c << s], i.e. the
 * level sees labels[:, ::2**s, ::2**s, ::2**s].  Level l is an entry of a HOST table: its float32 logits (element
 * (n, c, v) at logits[n*stride_n + c*stride_c + v*stride_v], v the flat index over d x h x w), its extents and its
 * shift; (d - 1) << s <= D - 1 (and likewise for h, w) is required, which holds for d = ceil(D / 2**s); level 0 has the
 * labels' extents and shift 0.
 *   loss_l as in ru3d_loss_fwd over the level's n * d * h * w voxels;  total = sum_l w_l * loss_l.
 * block: device float32 [2 * RU3D_DS_MAX_LEVELS + 1] (ru3d_ds_block_bytes): [0 .. 7] the level weights w_l, READ by the
 * device at execution time (rewrite them between the replays of a captured step); [8 .. 15] receive loss_l, [16] the
 * total.  state: ru3d_ds_state_bytes() bytes; receives per level the backward coefficients and the w_l of this forward;
 * the count of labels outside [0, C) - taken once, on level 0, which reads every label - sits at
 * ru3d_ds_state_bad_labels_offset() (the total and loss_0 are NaN then).  loss_out: 1 float32 on the device.
 * One sums launch over all levels (a block belongs to one level), one finalize workgroup that reduces the float64
 * partials of each level in a fixed order: no atomics, the same bits in every run. */
#define RU3D_DS_MAX_LEVELS 8
typedef struct ru3d_ds_level {
    const float* logits;
    int64_t stride_n, stride_c, stride_v;
    int32_t d, h, w, shift;
} ru3d_ds_level;
size_t ru3d_ds_state_bytes(void);
size_t ru3d_ds_state_bad_labels_offset(void);
size_t ru3d_ds_block_bytes(void);
size_t ru3d_ds_loss_workspace_bytes(const ru3d_ds_level* levels, int num_levels, int n);
int ru3d_ds_loss_fwd(const ru3d_ds_level* levels, int num_levels, const void* labels, int label_dtype, int n, int D, int H,
                     int W, int num_classes, int kind, float gamma, const float* weight_v, float alpha, float beta,
                     float smooth, float* block, void* state, float* loss_out, void* ws, size_t ws_bytes, void* stream);
/* dlogits[l] (HOST array of num_levels device pointers; float32, the strides of level l's logits) =
 * w_l * grad_out[0] * d loss_l / d logits_l for every level in one launch; w_l and the coefficients from `state` as the
 * forward left them, grad_out a device float32 or NULL for 1. */
int ru3d_ds_loss_bwd(const ru3d_ds_level* levels, void* const* dlogits, int num_levels, const void* labels,
                     int label_dtype, int n, int D, int H, int W, int num_classes, float gamma, const void* state,
                     const float* grad_out, void* stream);
/* the same with an ignore label (semantics: the comment of ru3d_loss_ignore_fwd) */
int ru3d_ds_loss_ignore_fwd(const ru3d_ds_level* levels, int num_levels, const void* labels, int label_dtype, int n, int D,
                            int H, int W, int num_classes, int has_ignore, int ignore_label, int kind, float gamma,
                            const float* weight_v, float alpha, float beta, float smooth, float* block, void* state,
                            float* loss_out, void* ws, size_t ws_bytes, void* stream);
int ru3d_ds_loss_ignore_bwd(const ru3d_ds_level* levels, void* const* dlogits, int num_levels, const void* labels,
                            int label_dtype, int n, int D, int H, int W, int num_classes, int has_ignore,
                            int ignore_label, float gamma, const void* state, const float* grad_out, void* stream);

/* ------------------------------------------------------------------ surface meshes */
/* The anatomy as closed triangle meshes: the faces between a set voxel and an unset one of a packed mask (the
 * "cuberille"), Taubin smoothing on the lattice's own edge graph, area and enclosed volume.  Masks are the packed masks
 * of the morphology section; everything outside the volume reads as unset.  X*Y*Z < 2^31, V < 2^31, 2Q < 2^31.
 *
 * Lattice corner (i, j, k), 0 <= i <= X, 0 <= j <= Y, 0 <= k <= Z, is the point (i - 0.5, j - 0.5, k - 0.5) in voxel
 * coordinates (voxel centres sit on integers, as in NIfTI).
 *   Vertices.   A corner is a vertex iff the eight voxels around it, M[i-1..i][j-1..j][k-1..k], are neither all set nor
 *               all unset.  Vertices are numbered in corner order, i outermost, k fastest.  corners: int32 [V][3].
 *   Quads.      exposed[x][y][z][d], d in the order -x, +x, -y, +y, -z, +z, is true iff the voxel is set and its
 *               neighbour in direction d is unset or outside.  Quads are numbered in element order of that array (x
 *               outermost, d fastest).  For direction +u, with (u, v, w) a cyclic permutation of (x, y, z), the quad's
 *               corners q0 .. q3 are the voxel's far-u corners with (v, w) offsets (0,0), (1,0), (1,1), (0,1); for -u
 *               the near-u corners with (0,0), (0,1), (1,1), (1,0).
 *   Triangles.  Quad q gives triangles 2q = (q0, q1, q2) and 2q + 1 = (q0, q2, q3): counter-clockwise seen from
 *               outside in index space.  faces: int32 [2Q][3] of vertex numbers.  The surface is closed and consistently
 *               oriented: every undirected edge is used equally often in both directions.
 *   Edge graph. neighbours: int32 [V][6], same direction order: the vertex number of the corner one lattice step away
 *               if the four voxels around that lattice edge are neither all set nor all unset, else -1.  Quad diagonals
 *               are not edges of this graph.  The table is symmetric and every vertex has at least three neighbours.
 *   Smoothing.  Positions are float64 [V][3], initially corners - 0.5.  One umbrella step with factor f: s = 0, then
 *               the present neighbours' positions added to it in direction order, m = their number,
 *                   q[v] = fl(p[v] + fl(f * fl(fl(s / m) - p[v])))      per component, no fused multiply-add
 *               (m = 0: q[v] = p[v]).  Taubin smoothing of n iterations is n times (step with lam, then step with mu).
 *               Expression and order are fixed, so the result can be compared with == against a restatement in numpy.
 *               Smoothing runs in index space with uniform weights whatever the voxel spacing; an affine is applied
 *               to the smoothed positions afterwards.
 *   Measures.   Over float64 positions and a face list: area = fl(0.5 * S), S = the sum over the faces of
 *               |(p1 - p0) x (p2 - p0)|; volume = fl(T / 6), T = the sum of p0 . (p1 x p2).  Both sums run in float64
 *               over a fixed partition in a fixed order: the same bits in every run and under every CU budget.  On the
 *               unsmoothed mesh in voxel coordinates volume == popcount(M) and area == Q exactly.
 *
 * ru3d_mesh_count: counts (device int64 [2]) = (V, Q).  ru3d_mesh_emit: the same counts again, whatever the capacities,
 * and the first vcap vertices (corners, neighbours) and the first qcap quads (faces: 2 * qcap triangles); nothing is
 * written at or beyond a capacity, so counts above them mean the buffers were too small.  A capacity of 0 skips that
 * output (its pointers may then be NULL).  When V or 2Q is not below 2^31 the counts are still exact and the buffers'
 * contents are not defined.  The two calls are independent: emit needs nothing of count's but the caller's sizes.
 * Workspace (ru3d_mesh_workspace_bytes): the corner flags as packed words of Z + 1 bits per (i, j) row, an int32
 * count of the vertices in front of each such word, and one int per 256 words of flags and of the mask. */
size_t ru3d_mesh_workspace_bytes(int X, int Y, int Z);
int ru3d_mesh_count(const uint64_t* bits, int X, int Y, int Z, int64_t* counts, void* ws, size_t ws_bytes, void* stream);
int ru3d_mesh_emit(const uint64_t* bits, int X, int Y, int Z, int32_t* corners, int32_t* neighbours, int64_t vcap,
                   int32_t* faces, int64_t qcap, int64_t* counts, void* ws, size_t ws_bytes, void* stream);
/* One umbrella step dst = step(src) over V vertices, not in place.  An entry of `neighbours` outside 0 .. V - 1 counts
 * as absent. */
int ru3d_mesh_smooth(const double* src, double* dst, const int32_t* neighbours, int64_t V, double factor, void* stream);
/* out (device float64 [2]) = (area, volume) of F triangles over V positions; a face that names a vertex outside
 * 0 .. V - 1 adds nothing.  Workspace: two doubles per 2048 faces. */
size_t ru3d_mesh_measure_workspace_bytes(int64_t F);
int ru3d_mesh_measure(const double* vertices, int64_t V, const int32_t* faces, int64_t F, double* out, void* ws,
                      size_t ws_bytes, void* stream);

/* ------------------------------------------------------------------ rendering: slice tiles and shaded surface views */
/* Pictures of a case that lives in HBM (csrc/render.hip): RGB8 canvases [H, W, 3], row-major, written by the device
 * and downloaded as they are.  The arithmetic below is the contract; visualize.py restates it in numpy and the two
 * routes are compared with ==.  Integers wherever possible; every float64 expression is evaluated as written, one
 * rounding per operation (fl), no fused multiply-add, no transcendental function.  Volumes have fewer than 2^31
 * elements.  Colour tables are device arrays of 256 RGBA rows (uint8 [256][4]).
 *
 * ru3d_render_tiles: one launch paints a DEVICE table of num_tiles (1 .. RU3D_RENDER_MAX_TILES) records into the canvas.
 *   A record shows slice `index` of axis `axis` of its volume; the two other axes in ascending order are the tile's
 *   row axis and column axis (matplotlib's imshow of volume[index, :, :]).  Tile pixel (r, c), 0 <= r < h, 0 <= c < w,
 *   is canvas pixel (y0 + r, x0 + c); pixels outside the canvas are not stored.  It shows the voxel whose in-plane
 *   indices are floor(fl(origin[0] + fl(r * step[0]))) and floor(fl(origin[1] + fl(c * step[1]))) - nearest voxel on a
 *   grid whose step is pixel size / voxel size, which is how anisotropic spacing becomes square pixels; an index
 *   outside the volume gives a black pixel.
 *   Base colour.  RU3D_TILE_F32: volume is the fp32 case layout [X][Y][Z][C], value v of channel `channel` as float64,
 *   t = fl(fl(v - vmin) / fl(vmax - vmin)), then t = 0 unless t > 0, t = 1 if t > 1 (NaN and 0/0 become 0),
 *   g = floor(fl(fl(255 * t) + 0.5)) on all three channels.  RU3D_TILE_U8: volume is uint8 [X][Y][Z], colour = the
 *   RGB of table[value] (alpha ignored).
 *   Overlays, 0 then 1, each a uint8 [X][Y][Z] volume of the same shape or NULL: l = its value at the voxel,
 *   (R, G, B, A) = overlay_table[l].  Nothing is drawn when A == 0, nor in mode RU3D_OVERLAY_OUTLINE unless l differs
 *   from the overlay's value at one of the voxel's four in-plane neighbours (a neighbour outside the volume reads 0).
 *   Otherwise every channel becomes (A * colour + (255 - A) * channel + 127) / 255 in integers.
 *   A record with a bad axis, index, channel, kind or extent, or a RU3D_TILE_F32 volume that is not 4-byte aligned,
 *   paints nothing.  The rectangles of one table must not overlap inside the canvas: tiles are painted by different
 *   workgroups in no order, and where two rectangles share a pixel its colour is that of either tile.
 * ru3d_render_surface: orthographic ray cast of a uint8 label volume [X][Y][Z] into rgb [H][W][3] and depth int32
 *   [H][W].  Coordinates are VOXEL units: voxel (i, j, k) is the box [i, i+1) x [j, j+1) x [k, k+1); the host divides
 *   its millimetre vectors by the spacing per component.  Sample n = 0 .. num_steps - 1 of pixel (row v, column u)
 *   sits at q_c = fl(fl(fl(o_c + fl(u * du_c)) + fl(v * dv_c)) + fl(n * dw_c)) per component c and reads the label of
 *   voxel floor(q); outside the volume the label is 0.  Label L is drawn iff L != 0 and table[L].A != 0.
 *   A surface event is a sample whose label L is drawn and differs from the previous sample's label (0 in front of
 *   sample 0).  At an event in voxel p: g_c = the sum over the offsets d in {-1, 0, 1}^3 of d_c * [label(p + d) == L]
 *   (three integers in -9 .. 9), m_c = fl(-g_c / spacing_c), dot = fl(fl(fl(m_0 l_0) + fl(m_1 l_1)) + fl(m_2 l_2)) with
 *   the light vector l, len2 the same expression with m in place of l;
 *       shade = fl(ambient + fl(fl(diffuse * max(dot, 0)) / sqrt(len2))),   len2 == 0: shade = fl(ambient + diffuse).
 *   Front to back, starting from T = 1 and C = (0, 0, 0), with a = fl(A / 255):
 *       C_c = fl(C_c + fl(fl(fl(T * a) * shade) * colour_c)),  then  T = fl(T * fl(1 - a));
 *   the ray ends when T < 1/256 or after the last sample.  Finally C_c = fl(C_c + fl(T * background_c)) and the pixel
 *   is floor(fl(min(max(C_c, 0), 255) + 0.5)).  depth = n of the first event, -1 without one.
 *   ru3d_render_surface_prepare fills the workspace for one (volume, table) pair - the drawn voxels as a packed mask
 *   in the layout of the morphology section, and one byte per 8 x 8 x 8 brick that holds a drawn voxel - and any
 *   number of views may follow.  The kernel does not visit every sample.  What it leaves out, and why that cannot
 *   change the picture: (1) samples outside n_lo <= n < n_hi of a slab test against the volume in real arithmetic from
 *   fl(fl(o + fl(u du)) + fl(v dv)), widened by two samples - rounding is monotone and 0 and the extents are
 *   representable, so a sample the contract places inside the volume lies within 2^-32 samples of that interval;
 *   (2) samples n + 1 .. n + j - 1 behind a sample n that lies in a brick without a drawn voxel, where j comes from an
 *   estimate of the brick's exit and is used only if the contract's own position of sample n + j - 1 lies in the same
 *   brick - every component of q is monotone in n, so all samples between lie in it too and read an undrawn label
 *   (without that check the estimate is wrong by many samples where |dw_c| is below an ulp of q_c, as for the
 *   cos(270 deg) of a lateral view); (3) the label byte of a sample whose mask bit is clear: it is not drawn, and a drawn
 *   label always differs from an undrawn one.  Every visited sample is placed by the expression above from its n.
 *   The view travels in the kernel arguments.  `ws` is 8-byte aligned in both calls. */
#define RU3D_RENDER_MAX_TILES 256
enum { RU3D_TILE_F32 = 0, RU3D_TILE_U8 = 1 };
enum { RU3D_OVERLAY_FILL = 0, RU3D_OVERLAY_OUTLINE = 1 };
typedef struct ru3d_render_tile {
    const void* volume;
    const uint8_t* table;            /* RU3D_TILE_U8 only */
    const uint8_t* overlay[2];       /* NULL: none */
    const uint8_t* overlay_table[2];
    double vmin, vmax;               /* RU3D_TILE_F32 only */
    double origin[2], step[2];       /* row axis, column axis */
    int32_t x0, y0, w, h;
    int32_t X, Y, Z, C, channel, kind, axis, index;
    int32_t overlay_mode[2];
} ru3d_render_tile;
typedef struct ru3d_render_view {
    double o[3], du[3], dv[3], dw[3]; /* voxel units; all finite */
    double spacing[3];                /* positive */
    double light[3];
    double ambient, diffuse;
    double background[3];
    int32_t num_steps, reserved;
} ru3d_render_view;
int ru3d_render_tiles(const ru3d_render_tile* tiles, int num_tiles, uint8_t* canvas, int H, int W, void* stream);
size_t ru3d_render_surface_workspace_bytes(int X, int Y, int Z);
int ru3d_render_surface_prepare(const uint8_t* labels, int X, int Y, int Z, const uint8_t* table, void* ws, size_t ws_bytes,
                                void* stream);
int ru3d_render_surface(const uint8_t* labels, int X, int Y, int Z, const uint8_t* table, const ru3d_render_view* view,
                        uint8_t* rgb, int32_t* depth, int H, int W, const void* ws, size_t ws_bytes, void* stream);

/* ------------------------------------------------------------------ patch sampling + augmentation */
/* The reference's training transform chain on the device: RandomRescaleCrop -> RandomMirror ->
 * RandomContrast -> RandomBrightness -> RandomGamma -> ToTensor (transform.py:573-652, 279-301, 176-259, 156-163;
 * nb_train_iia.py:30-39).  The HOST makes the random draws (in the reference's order) and passes them here; the
 * kernels are deterministic.  image: fp32 volume [X][Y][Z][C] (the reference's channels-last case layout), label:
 * [X][Y][Z] uint8 or int64.  out_image: fp32 [C][px][py][pz] (ToTensor layout = one NCDHW sample), out_label: int64
 * [px][py][pz].  Resampling restates scipy.ndimage.zoom(order=1): corner-aligned linear interpolation in float64. */
typedef struct ru3d_patch_params {
    int32_t lo[3];      /* crop box lower corner in the volume, per axis (may lie outside: constant padding)      */
    int32_t before[3];  /* crop box size = round(patch / scale), transform.py:617                                  */
    int32_t patch[3];   /* output patch size                                                                       */
    int32_t flip[3];    /* RandomMirror: reverse this output axis                                                   */
    float image_cval;   /* image_pad_cval                                                                           */
    int32_t label_cval; /* label_pad_cval                                                                           */
    int32_t do_contrast, do_brightness, do_gamma;
    float contrast, brightness, gamma; /* the drawn factors                                                         */
    float gamma_eps;    /* adjust_gamma's epsilon (1e-7), transform.py:188                                          */
} ru3d_patch_params;
size_t ru3d_augment_workspace_bytes(int px, int py, int pz);
/* mask (1 device uint32): bit min(v, 31) set for every label value v inside the crop box (pad value included). */
int ru3d_augment_label_presence(const void* label, int label_dtype, int X, int Y, int Z, const int32_t* lo,
                                const int32_t* before, int label_cval, uint32_t* mask, void* stream);
/* label / out_label may both be NULL (image only), or image / out_image (label only).  presence_mask: device uint32 from the call above (the label rule
 * of transform.py:47-48 needs the number of classes in the crop); NULL = treat as >= 3 classes. */
int ru3d_augment_patch(const float* image, const void* label, int label_dtype, int X, int Y, int Z, int C,
                       const ru3d_patch_params* p, const uint32_t* presence_mask, float* out_image, int64_t* out_label,
                       void* ws, size_t ws_bytes, void* stream);

/* The same patch through a free-form spatial transform: rotation, the per-axis zoom above and a cubic B-spline elastic
 * displacement.  All of the geometry is float64.  Patch P = p->patch, output voxel o, mirrored index
 * o'_d = p->flip[d] ? P_d - 1 - o_d : o_d, centred u = o' - (P - 1) / 2:
 *
 *     s(o) = centre + matrix . (u + D(o'))          source coordinate in voxels of the volume
 *
 * The host folds the crop box into the two: centre = lo + (before - 1) / 2, matrix = R . diag(step) with
 * step_d = (before_d - 1) / (P_d - 1) (0 when P_d == 1) and R = Rz(az) . Ry(ay) . Rx(ax), right-handed
 * (Rx(a) = [[1,0,0],[0,cos a,-sin a],[0,sin a,cos a]]).  R = I and D = 0 give lo + o' * step, the coordinate of
 * ru3d_augment_patch.  D, in patch voxels, comes from control vectors phi = lattice[3][nx][ny][nz] (float32, device) with
 * n_d = ceil((P_d - 1) / g_d) + 3 for a control spacing of g_d = spacing[d] patch voxels: with t_d = o'_d / g_d,
 * i_d = floor(t_d), f_d = t_d - i_d
 *
 *     D(o') = sum over a, b, c in 0..3 of B_a(fx) B_b(fy) B_c(fz) * phi[:][ix + a][iy + b][iz + c]
 *     B_0 = (1-f)^3 / 6,  B_1 = (3f^3 - 6f^2 + 4) / 6,  B_2 = (-3f^3 + 3f^2 + 3f + 1) / 6,  B_3 = f^3 / 6
 *
 * (the uniform cubic B-spline; a constant lattice is a pure shift; where (P_d - 1) / g_d is whole the last voxel of the
 * axis has i_d + 3 == n_d with weight B_3(0) = 0; that tap reads the last control point).  Sampling at s, clamped to [-2, extent + 1] per axis:
 * i0 = floor(s), w = s - i0, the 8 neighbours i0 + {0, 1}; a neighbour outside the volume contributes image_cval /
 * label_cval (the volume continued by the constant); float64 lerps along axis 0, then 1, then 2, float32 result; labels by
 * the rule of ru3d_augment_patch with the presence mask of the drawn (axis-aligned) crop box.  p->lo / p->before are not
 * read.  Workspace, per-block partials and the intensity chain are those of ru3d_augment_patch.
 * A workgroup keeps the lattice collapsed along x - [3][ny][nz] float64 - and one [3][nz] row per wave in LDS (60 KB at
 * most): a lattice with (ny + 4) * nz > RU3D_SPATIAL_MAX_YZ is refused.  128^3 at g = 16 is 15 * 11, 256^3 at g = 16
 * 23 * 19, 128^3 at g = 4 39 * 35 (all accepted); 192^3 at g = 4 is 55 * 51 (refused). */
#define RU3D_SPATIAL_MAX_YZ 2560
typedef struct ru3d_spatial_params {
    double centre[3];   /* c                                                                                        */
    double matrix[9];   /* M, row-major                                                                             */
    int32_t lattice[3]; /* control points per axis; all 0 = no displacement                                         */
    int32_t spacing[3]; /* g: patch voxels per lattice cell (>= 4); read when there is a lattice                    */
} ru3d_spatial_params;
int ru3d_augment_patch_spatial(const float* image, const void* label, int label_dtype, int X, int Y, int Z, int C,
                               const ru3d_patch_params* p, const ru3d_spatial_params* sp,
                               const float* lattice /* device, [3][nx][ny][nz]; NULL without a lattice */,
                               const uint32_t* presence_mask, float* out_image, int64_t* out_label, void* ws,
                               size_t ws_bytes, void* stream);

/* The class-location index of a case, for foreground-oversampled patches: with probability p the sampler centres the
 * crop box on a voxel drawn from this index instead of drawing boxes until the class happens to be inside one.  label:
 * uint8 or int64 [X, Y, Z] (RU3D_LABEL_U8 / RU3D_LABEL_I64), linear index i = (x * Y + y) * Z + z < 2^31.  All outputs
 * are device memory:
 *   counts[c]        the number of voxels with value c, c in 0 .. 31; a value below 0 or above 31 is counted nowhere and
 *                    appears nowhere;
 *   boxes[c]         {x0, x1, y0, y1, z0, z1} of those voxels, low end inclusive, high end exclusive; zeros when
 *                    counts[c] == 0;
 *   locations[c][j]  for j < m = min(counts[c], max_per_class): the linear index of the voxel of class c whose rank among
 *                    the class's voxels in raster order is (j * counts[c]) / m (64-bit integer division) - the complete
 *                    raster-ordered list when the class has at most max_per_class voxels, an evenly rank-strided
 *                    subsample otherwise: np.flatnonzero(label == c)[(np.arange(m) * n) // m].  Slots j >= m hold -1.
 * 1 <= max_per_class <= RU3D_CLASS_INDEX_MAX_PER_CLASS.  Integer arithmetic only, and no atomic decides a position: the
 * result is the same bits in every run.  Workspace: 32 ints per 2048 voxels.  The volume is read twice. */
#define RU3D_CLASS_INDEX_CLASSES 32
#define RU3D_CLASS_INDEX_MAX_PER_CLASS (1 << 20)
size_t ru3d_class_index_workspace_bytes(int X, int Y, int Z); /* 0 when the shape is refused */
int ru3d_class_index(const void* label, int label_dtype, int X, int Y, int Z, int max_per_class,
                     int64_t* counts /* [32] */, int32_t* boxes /* [32][6] */,
                     int32_t* locations /* [32][max_per_class] */, void* ws, size_t ws_bytes, void* stream);

/* Image-quality augmentation of a sampled patch, between the resampling above and the intensity chain: Gaussian noise,
 * Gaussian blur, simulated low resolution, in that order, each on the image only and on all C channels of the patch
 * image[C][px][py][pz] (fp32, in place) with one parameter set.  The HOST draws the parameters; the kernels are
 * deterministic and restate the numpy twins of degrade.py.
 *
 *   noise    Philox4x32-10 (multipliers 0xD2511F53 / 0xCD9E8D57, Weyl constants 0x9E3779B9 / 0xBB67AE85) with key
 *            noise_key and counter (j, 0, 0, 0) gives x0..x3; in float64 u_a = (x0 + 0.5) * 2^-32, u_b = (x1 + 0.5) * 2^-32,
 *            n0 = sqrt(-2 ln u_a) cos(2 pi u_b), n1 = sqrt(-2 ln u_a) sin(2 pi u_b), n2 / n3 from x2 / x3 alike.  The voxel
 *            with linear index i over [C][px][py][pz] takes normal i & 3 of call j = i >> 2:
 *            out = float32(float64(x) + sqrt(noise_variance) * n), one rounding.
 *   blur     scipy.ndimage.gaussian_filter(x, blur_sigma) with its defaults (mode 'reflect': ... b a | a b ..., truncate 4),
 *            one sigma for the three axes: radius r = int(4 sigma + 0.5), weights exp(-t^2 / 2 sigma^2) normalised in
 *            float64, passes along x, then y, then z, each accumulated in float64 (the centre, then the pairs of taps from
 *            the outermost inwards) and stored as float32.  r > RU3D_DEGRADE_MAX_RADIUS and r > min(px, py, pz) (a
 *            single reflection would not suffice) are refused.
 *   low-res  nearest-neighbour down to the grid n_d = max(round-half-even(P_d * low_res_zoom), 2), order 1 back up to P,
 *            scipy.ndimage.zoom's corner-aligned coordinates: output voxel o reads low-grid coordinate
 *            t = o * ((n - 1) / (P - 1)) (the ratio formed once in float64), low-grid voxel l is source voxel
 *            floor(l * ((P - 1) / (n - 1)) + 0.5); the 8 sources are weighted in float64 (value times the x, y and z
 *            weight in turn, summed with the last axis fastest) and rounded to float32 once.  0 < zoom <= 1, P_d >= 2;
 *            zoom 1 returns the input bits.  One fused gather: no low-resolution volume is materialised.
 *
 * The call ends by writing the per-block {sum, min, max} partials of the FINAL image to `part`
 * ((px * py * pz + 255) / 256 triples of doubles, block b = voxels 256 b .. 256 b + 255 of every channel, summed in a
 * fixed order): the layout ru3d_augment_patch leaves in its workspace, so that ru3d_augment_intensity describes the
 * degraded image.  With no op switched on only the partials are written.  `ws` (device,
 * ru3d_augment_degrade_workspace_bytes) holds the ping-pong image and the low-res tables and must not overlap `part`. */
#define RU3D_DEGRADE_MAX_RADIUS 16
typedef struct ru3d_degrade_params {
    int32_t do_noise, do_blur, do_low_res;
    uint32_t noise_key[2]; /* Philox key (k0, k1)                                                                   */
    int32_t reserved;
    double noise_variance; /* >= 0                                                                                   */
    double blur_sigma;     /* > 0, in voxels                                                                         */
    double low_res_zoom;   /* in (0, 1]                                                                              */
} ru3d_degrade_params;
size_t ru3d_augment_degrade_workspace_bytes(int C, int px, int py, int pz);
int ru3d_augment_degrade(float* image /* [C][px][py][pz], in place */, int C, int px, int py, int pz,
                         const ru3d_degrade_params* p, void* ws, size_t ws_bytes, double* part, void* stream);
/* The intensity chain of ru3d_augment_patch on its own: contrast about the mean, brightness about the minimum, gamma on
 * the [min, max] range of image[count] (fp32, in place), the statistics taken from `nparts` {sum, min, max} triples (what
 * ru3d_augment_patch / _spatial leave at the start of their workspace, or ru3d_augment_degrade in `part`).  Reads the
 * do_* flags, factors and gamma_eps of p; nothing is launched when no flag is set. */
int ru3d_augment_intensity(float* image, int64_t count, const double* part, int nparts, const ru3d_patch_params* p,
                           void* stream);

/* ------------------------------------------------------------------ optimizer --------------- */
/* torch.optim.Adam step (nb_train_iia.py:18 defaults), fused over one flat fp32 parameter run.
 * grad may be bf16/f32 (grad_dtype); bias corrections are passed in by the host. */
int ru3d_adam_step(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, int64_t count,
                   float lr, float beta1, float beta2, float eps, float bias_corr1, float bias_corr2,
                   float grad_scale, void* stream);

/* The same update for MANY parameter tensors in one launch.  `tensors` and `block_map` are DEVICE arrays:
 * block b of the grid updates elements [chunk*chunk_elems, +chunk_elems) of tensors[block_map[2b]] with
 * chunk = block_map[2b+1].  Tensors whose grad pointer is NULL are skipped (no gradient this step). */
typedef struct ru3d_adam_tensor {
    float* param;
    const float* grad;
    float* exp_avg;
    float* exp_avg_sq;
    int64_t count;
} ru3d_adam_tensor;
int ru3d_adam_multi(const ru3d_adam_tensor* tensors, const int32_t* block_map, int nblocks, int chunk_elems,
                    float lr, float beta1, float beta2, float eps, float bias_corr1, float bias_corr2,
                    float grad_scale, void* stream);

/* ru3d_adam_multi with the per-step scalars read from device memory - hyper[8] = {lr, beta1, beta2, eps, bias_corr1,
 * bias_corr2, grad_scale, sqrtf(bias_corr2)} - so that a launch captured in a hipGraph follows the step count and the learning-rate
 * schedule: the host rewrites the 32 bytes before each replay. */
int ru3d_adam_multi_dev(const ru3d_adam_tensor* tensors, const int32_t* block_map, int nblocks, int chunk_elems,
                        const float* hyper, void* stream);

/* The loss scaler of fp16 training held on the DEVICE (32 bytes), so that a whole fp16 step - scaled loss, backward,
 * overflow check, Adam, scaler update - is a fixed launch sequence a hipGraph can replay (the reference trains with apex
 * O1: trainer.py:492-493, 538-542).  ru3d_grad_scale_check(scale = 1) writes found_inf; ru3d_adam_multi_amp is
 * ru3d_adam_multi_dev that skips itself on found_inf != 0, multiplies the gradients by inv_scale and takes the Adam step
 * number from hyper[5] (an int32 in the float slot: steps taken before the capture) + steps + 1, with hyper[4] / hyper[7]
 * the residuals beta - (float)beta of the two betas (bias corrections in double); ru3d_amp_update then
 * applies apex's schedule (overflow: scale *= backoff, tracker = 0, skipped++; clean: steps++, tracker++, after
 * growth_interval clean steps scale *= growth) and clears found_inf.  The host reads the block back when it wants to
 * know (state_dict, logging), not every step. */
typedef struct ru3d_amp_state {
    float scale, inv_scale, found_inf;
    int32_t tracker, skipped, steps, reserved0, reserved1;
} ru3d_amp_state;
int ru3d_adam_multi_amp(const ru3d_adam_tensor* tensors, const int32_t* block_map, int nblocks, int chunk_elems,
                        const float* hyper, const ru3d_amp_state* amp, void* stream);
int ru3d_amp_update(ru3d_amp_state* amp, float growth_factor, float backoff_factor, int growth_interval, float min_scale,
                    float max_scale, void* stream);

/* The global L2 norm of every gradient a table names (same table / block-map layout as ru3d_adam_multi; only grad and
 * count are read) and the clipping coefficient of torch.nn.utils.clip_grad_norm_(norm_type=2, error_if_nonfinite=False),
 * without atomics and in a fixed order:
 *   ru3d_grad_sumsq:       partials[b] = float64 sum of the float64 squares of block b's chunk, 0 for a row whose grad is
 *                          NULL (partials: nblocks doubles).  Several tables (param groups) write into consecutive
 *                          stretches of one partials array.
 *   ru3d_grad_norm_finish: one workgroup adds npartials doubles and writes the norm block out[2] (device floats):
 *                            out[0] = total = (float)(grad_scale * sqrt(sum))     the norm of the TRUE gradients when
 *                                                                                 grad_scale is the fp16 path's 1 / loss_scale
 *                            out[1] = coef  = min(1, max_norm / (total + 1e-6f))  NaN stays NaN (torch.clamp); an inf
 *                                                                                 total gives 0
 *                          hyper != NULL: grad_scale is read from hyper[6] of a captured step's scalar row instead.
 *   ru3d_grad_norm:        both launches for one table (npartials = nblocks).
 *   ru3d_grad_scale_dev:   g *= *coef in place over the table's gradients (clip_grad_norm_ on its own); writes nothing
 *                          when *coef == 1. */
int ru3d_grad_sumsq(const ru3d_adam_tensor* tensors, const int32_t* block_map, int nblocks, int chunk_elems,
                    double* partials, void* stream);
int ru3d_grad_norm_finish(const double* partials, int npartials, float grad_scale, const float* hyper, float max_norm,
                          float* out, void* stream);
int ru3d_grad_norm(const ru3d_adam_tensor* tensors, const int32_t* block_map, int nblocks, int chunk_elems,
                   double* partials, float grad_scale, float max_norm, float* out, void* stream);
int ru3d_grad_scale_dev(const ru3d_adam_tensor* tensors, const int32_t* block_map, int nblocks, int chunk_elems,
                        const float* coef, void* stream);

/* torch.optim.SGD (dampening = 0, maximize = False) over a ru3d_adam_tensor table, one launch per param group:
 *   gh = g * grad_scale * coef;  d = gh + weight_decay * p;  b = momentum * b + d  (momentum != 0; a zero buffer gives
 *   torch's first step b = d);  u = nesterov ? d + momentum * b : b  (u = d when momentum == 0);  p -= lr * u.
 * The momentum buffer b travels in the table's exp_avg slot (NULL when momentum == 0), exp_avg_sq is NULL.  coef: the
 * device float ru3d_grad_norm_finish wrote (out + 1), or NULL for an unclipped step - the coefficient is multiplied in
 * while the gradient is read, the gradients themselves are not written.  No fused multiply-adds: vector path, scalar
 * path, this form and the _dev form give identical bits.
 * _dev: hyper[8] = {lr, momentum, weight_decay, nesterov (0 / 1), -, -, grad_scale, -} from device memory (a captured
 * step; the host rewrites the row before each replay). */
int ru3d_sgd_multi(const ru3d_adam_tensor* tensors, const int32_t* block_map, int nblocks, int chunk_elems, float lr,
                   float momentum, float weight_decay, int nesterov, float grad_scale, const float* coef, void* stream);
int ru3d_sgd_multi_dev(const ru3d_adam_tensor* tensors, const int32_t* block_map, int nblocks, int chunk_elems,
                       const float* hyper, const float* coef, void* stream);

/* torch.optim.AdamW: p *= 1 - lr * weight_decay, then ru3d_adam_multi's recurrence on gh = g * grad_scale * coef (coef as
 * for ru3d_sgd_multi).  _dev: hyper[8] = {lr, beta1, beta2, eps, bias_corr1, bias_corr2, grad_scale, weight_decay}; slot 7
 * carries the decay, so both forms take sqrtf(bias_corr2) on the device and stay bit-equal to each other. */
int ru3d_adamw_multi(const ru3d_adam_tensor* tensors, const int32_t* block_map, int nblocks, int chunk_elems, float lr,
                     float beta1, float beta2, float eps, float weight_decay, float bias_corr1, float bias_corr2,
                     float grad_scale, const float* coef, void* stream);
int ru3d_adamw_multi_dev(const ru3d_adam_tensor* tensors, const int32_t* block_map, int nblocks, int chunk_elems,
                         const float* hyper, const float* coef, void* stream);

/* ru3d_adam_multi / ru3d_adam_multi_dev (same scalars, same hyper row) with the clipping coefficient multiplied into
 * the gradient as it is read; with *coef == 1 or coef == NULL the result is ru3d_adam_multi's, bit for bit. */
int ru3d_adam_multi_clip(const ru3d_adam_tensor* tensors, const int32_t* block_map, int nblocks, int chunk_elems,
                         float lr, float beta1, float beta2, float eps, float bias_corr1, float bias_corr2,
                         float grad_scale, const float* coef, void* stream);
int ru3d_adam_multi_clip_dev(const ru3d_adam_tensor* tensors, const int32_t* block_map, int nblocks, int chunk_elems,
                             const float* hyper, const float* coef, void* stream);

/* conv3d input gradient FOLLOWED by the InstanceNorm + LeakyReLU backward of the tensor it differentiates (ResBlock
 * backward, network.py:411-416 read backwards: da = conv2^T(dy); dyn = d/dy1 of lrelu(IN(y1)) given da) - the
 * mirror image of ru3d_conv3d_fwd_in.  `act` = lrelu(IN(y1)) as the forward produced it, mean / scale = that
 * InstanceNorm's statistics; da receives the conv's result (gradient wrt act), dyn the gradient wrt y1.  On the
 * shapes of the sliding 32-channel kernel the two sums the backward needs (sum g', sum g' xhat) are taken in the
 * conv's epilogue and the separate reduction pass over (da, act) is not run; elsewhere the call is
 * ru3d_conv3d_dgrad + ru3d_in_lrelu_bwd.  Workspace: ru3d_conv3d_dgrad_in_bwd_workspace_bytes. */
size_t ru3d_conv3d_dgrad_in_bwd_workspace_bytes(const ru3d_tensor* dy, const ru3d_tensor* da, int k, int stride,
                                                int dtype);
int ru3d_conv3d_dgrad_in_bwd(const ru3d_tensor* dy, const void* w_packed, const ru3d_tensor* act, const float* mean,
                             const float* scale, const ru3d_tensor* da, const ru3d_tensor* dyn, int k, int stride,
                             float slope, int dtype, void* ws, size_t ws_bytes, void* stream);
/* The apply pass of ru3d_in_lrelu_bwd alone (no residual form), with m12[n][c] = (mean g', mean g' xhat) given. */
int ru3d_in_lrelu_bwd_apply(const ru3d_tensor* gout, const ru3d_tensor* out, const float* mean, const float* scale,
                            const float* m12, const ru3d_tensor* dy, float slope, int zero_far, int dtype, void* stream);

/* ------------------------------------------------------------------ BatchNorm3d, training mode - */
/* Blocks built with norm_op=nn.BatchNorm3d (network.py:38-69 ResAttrBNUnet3D; nn.BatchNorm3d(C) defaults: affine,
 * running statistics, momentum 0.1, eps 1e-5) in training mode: statistics pooled over the batch, with the preceding
 * nn.Dropout3d's per-(n, c) factor d folded in (network.py:411-413).  Each direction is two calls with the pooled sums
 * handed back in between as doubles, so that a multi-GPU caller can all-reduce them (SyncBN; count is then the global
 * element count N * D * H * W summed over ranks).
 *   stats_pool:     pooled[2c] = sum_n d sum_v y, pooled[2c+1] = sum_n d^2 sum_v y^2     (ws: ru3d_reduce_workspace_bytes)
 *   stats_finalize: mu = pooled[2c] / count, var = pooled[2c+1] / count - mu^2 (biased), r = 1 / sqrt(var + eps);
 *                   a[n][c] = d r, b[n][c] = -mu r (x_hat = y a + b), fscale = gamma a, fshift = beta + gamma b;
 *                   running_mean / running_var (NULL: not tracked) move by `momentum` towards mu / the unbiased var.
 *                   c_real <= c: channels beyond it are zero padding (gamma = 1, beta = 0, no running update).
 *   affine_lrelu_fwd: out = LeakyReLU(y * scale[n][c] + shift[n][c] (+ res), slope)
 *   bwd_pool:       gpre = gout * LeakyReLU'(out) is stored; pooled[2c] = sum gpre (= dbeta of this rank),
 *                   pooled[2c+1] = sum gpre x_hat (= dgamma of this rank)
 *   bwd_apply:      dy = fscale * (gpre - pooled[2c] / count - x_hat * pooled[2c+1] / count); zero_far as in
 *                   ru3d_in_lrelu_bwd; ws: 2 * N * C floats. */
int ru3d_batchnorm_stats_pool(const ru3d_tensor* y, const float* drop_scale, double* pooled, void* ws, size_t ws_bytes,
                              int dtype, void* stream);
int ru3d_batchnorm_stats_finalize(const double* pooled, int n, int c, int c_real, double count, const float* drop_scale,
                                  const float* gamma, const float* beta, float eps, float momentum, float* running_mean,
                                  float* running_var, float* fscale, float* fshift, float* a, float* b, void* stream);
int ru3d_affine_lrelu_fwd(const ru3d_tensor* y, const float* scale, const float* shift, const ru3d_tensor* res,
                          const ru3d_tensor* out, float slope, int dtype, void* stream);
int ru3d_batchnorm_bwd_pool(const ru3d_tensor* gout, const ru3d_tensor* out, const ru3d_tensor* y, const float* a,
                            const float* b, const ru3d_tensor* gpre, double* pooled, void* ws, size_t ws_bytes,
                            float slope, int dtype, void* stream);
int ru3d_batchnorm_bwd_apply(const ru3d_tensor* gpre, const ru3d_tensor* y, const float* a, const float* b,
                             const float* fscale, const double* pooled, double count, const ru3d_tensor* dy, void* ws,
                             size_t ws_bytes, int zero_far, int dtype, void* stream);

/* Dynamic loss scaling of the fp16 mode (the reference's apex O1: trainer.py:492-493 amp.scale_loss, 538-542
 * amp.initialize): every gradient named by the table (same layout as ru3d_adam_multi; only grad / count are read) is
 * checked for inf / nan - *found_inf is set to 1.0 when one is found; the caller zeroes it beforehand - and multiplied
 * in place by `scale` (pass 1 / loss_scale; scale == 1 checks without writing). */
int ru3d_grad_scale_check(const ru3d_adam_tensor* tensors, const int32_t* block_map, int nblocks, int chunk_elems,
                          float scale, float* found_inf, void* stream);

/* ------------------------------------------------------------------ gradient exchange (RCCL) */
/* Data-parallel training: one process per GPU, one exchange per step - the mean of the parameter gradients over
 * ranks.  The reference has no distributed code (it pins one device, nb_train_iia.py:17); these entry points are
 * the build's own contract.  RCCL is resolved with dlopen at first use.
 *   rank 0:      ru3d_comm_unique_id(blob)      -> the host ships the 128-byte blob to every rank (any channel)
 *   every rank:  ru3d_comm_init(&comm, blob, world, rank, device)     (collective: all ranks must call it)
 *   per bucket:  ru3d_comm_allreduce(comm, buf, count, dtype, average, stream)   in place, enqueue-only
 *   at exit:     ru3d_comm_destroy(comm)
 * The communicator handle is the only state the library keeps, and it is owned by the caller. */
#define RU3D_COMM_ID_BYTES 128
int ru3d_comm_unique_id(void* id_out);
int ru3d_comm_init(void** comm_out, const void* unique_id, int world, int rank, int device);
/* buf: device buffer of `count` elements (RU3D_F32 or RU3D_BF16); average != 0 divides the sum by the world size. */
int ru3d_comm_allreduce(void* comm, void* buf, int64_t count, int dtype, int average, void* stream);
/* The same exchange as its two halves, each rank owning count_per_rank elements of the bucket (with 7
 * point-to-point xGMI links per GPU a ring all-reduce is bound by one link; reduce-scatter + all-gather lets RCCL use
 * its direct / mesh schedules and leaves room to run the optimizer on the owned shard between the two).  Both in place
 * on a bucket of world * count_per_rank elements: rank r's shard is elements [r * count_per_rank, (r + 1) * ..). */
int ru3d_comm_reduce_scatter(void* comm, void* buf, int64_t count_per_rank, int dtype, int average, void* stream);
int ru3d_comm_all_gather(void* comm, void* buf, int64_t count_per_rank, int dtype, void* stream);
/* 1 when librccl can be loaded in this process (no communicator is created, nothing collective happens): lets every
 * rank vote on the transport BEFORE any rank enters the collective ru3d_comm_init. */
int ru3d_comm_available(void);
int ru3d_comm_destroy(void* comm);
/* Kernel probe (bench.py's `roofline` object): between begin and end the library records a HIP-event pair on the launch
 * stream around the main kernel of every 3x3x3 stride-1 conv launch (forward or input gradient, any entry point) whose
 * output grid is n x d x h x w with cin -> cout channels; `end` waits for them and returns their number and the sum of
 * their durations.  Launches made while the stream is being captured into a graph are skipped. */
int ru3d_probe_begin(int n, int d, int h, int w, int cin, int cout);
int ru3d_probe_end(int* launches, double* total_ms);
/* Compute units the persistent conv kernels launched on a device may occupy (their grids are sized from it); 0 restores
 * the device's count.  A data-parallel rank leaves a few CUs to RCCL's reduction kernels on the side stream.  The value
 * belongs to the DEVICE (the CUs being divided are that device's): every entry point uses the budget of the device its
 * stream lives on.  ru3d_set_cu_budget / ru3d_get_cu_budget address the calling thread's current device. */
int ru3d_set_cu_budget_device(int device, int cus);
int ru3d_set_cu_budget(int cus);
int ru3d_get_cu_budget(void);
/* dst[i] = (dst_dtype)(src[i] * scale) on flat 16-byte-aligned device arrays, f32 <-> bf16: the copy-in / copy-out
 * of a bf16 gradient bucket (half the bytes over xGMI). */
int ru3d_flat_cast(const void* src, int src_dtype, void* dst, int dst_dtype, int64_t count, float scale, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* RU3D_H */
