// Internal geometry structs and launcher prototypes shared by the conv translation units.
#pragma once
#include "common.h"

namespace RU3D_NS {

struct ConvGeom {
    int N;
    int Di, Hi, Wi, Cin, ldx;    // input tensor (of the data-movement form, not of the nn.Module)
    int Do, Ho, Wo, Cout, ldy;   // output tensor
    int CoutPad;                 // generic layout: padded cout of the packed weight
    int ldr;                     // residual pitch (when res != NULL)
    int k, stride, pad;
    int transposed;              // 0 = gather form, 1 = transposed (fractionally strided) form
    int zero_far;                // write exact zeros on the last plane of each output axis
    int flip;                    // read weight tap (taps-1-tap): stride-1 dgrad as a gather conv
    // split (planar concat) layouts, see ru3d_tensor: 0 = dense.  Only the kernels of a decoder ResBlock on the
    // full-resolution level take them (conv_slide64 input, conv_slide32 pair output)
    int x_cseg = 0, y_cseg = 0;
    int64_t x_segstride = 0, y_segstride = 0;
};

struct WgradGeom {
    int N;
    int Di, Hi, Wi, Cin, ldx;    // "x" operand (gathered with stride/pad)
    int Do, Ho, Wo, Cout, lddy;  // "dy" operand (dense positions)
    int k, taps, stride, pad;
    int64_t s_o, s_i;            // element strides of dw for (cout, cin); tap stride is 1
    int64_t chunk_len;           // positions per chunk (filled by the launcher)
    int x_cseg = 0;              // split (planar concat) x, see ru3d_tensor: 0 = dense
    int64_t x_segstride = 0;
};

// batched weight packing (conv_generic.hip): both packed layouts, up to RU3D_PACK_MAX weights per launch
struct PackOne {
    const float* src;
    void* dst;
    int cin, cout, taps, mfma, cout_pad;   // cin / cout: PACKED (kernel-side) channel counts; mfma: 0 generic, 1 MFMA, 2 bias
    int co_real, co_pad, ci_real, ci_pad;  // channel padding per segment (pad == 0: none), see pack_src_index
    int64_t s_o, s_i, total;
};
struct PackBatch {
    int count;
    PackOne item[RU3D_PACK_MAX];
};
int pack_batch_launch(const PackBatch& b, int dtype, hipStream_t st);

// Fused packing of the two MFMA roles of one weight (forward + input gradient) from ONE read of the fp32 source:
// the source is [a][b][tap] (Conv3d: a = cout, b = cin; ConvTranspose3d: a = cin, b = cout); dst_a is the packed form
// whose output-channel dimension is a (Conv forward / ConvTranspose input gradient), dst_b the one whose output-channel
// dimension is b.  Either may be NULL.  adim / bdim are the PACKED (padded) extents, multiples of 32.
struct PackPair {
    const float* src;
    void* dst_a;
    void* dst_b;
    int adim, bdim, taps;
    int a_real, a_pad, b_real, b_pad;   // channel padding per segment (pad == 0: none), see pack_src_index
    int64_t s_a;                        // source stride of a (= real bdim * taps); b has stride taps, tap stride 1
};
struct PackPairBatch {
    int count;
    PackPair item[RU3D_PACK_MAX];
};
int pack_pair_launch(const PackPairBatch& b, hipStream_t st);
int unpad_weight_launch(const float* src, float* dst, int cout, int cin, int taps, int co_real, int co_pad, int ci_real,
                        int ci_pad, int cin_p, hipStream_t st);

// conv_generic.hip
int generic_cot(int cout);
int generic_cout_pad(int cout);
int conv_generic_launch(const void* x, const void* w, const float* bias, const void* res, void* y,
                        const ConvGeom& g, int dtype, int y_dtype, hipStream_t st);
int pack_generic_launch(const float* src, void* dst, int cin, int cout, int taps, int64_t s_o, int64_t s_i,
                        int flip, int dtype, hipStream_t st);
int wgrad_generic_chunks(const WgradGeom& g);
int wgrad_reduce_launch(const float* part, float* dw, int chunks, int taps, int cin, int cout, int64_t s_o, int64_t s_i,
                        hipStream_t st);
int wgrad_generic_launch(const void* x, const void* dy, float* dw, void* ws, int chunks, WgradGeom g, int dtype,
                         hipStream_t st);

// conv_mfma.hip (bf16 MFMA implicit GEMM)
bool mfma_conv_eligible(int cin, int cout, int k, int dtype, int y_dtype);
bool mfma_conv_geometry_ok(const ConvGeom& g);
size_t mfma_packed_bytes(int cin, int cout, int taps);
int pack_mfma_launch(const float* src, void* dst, int cin, int cout, int taps, int64_t s_o, int64_t s_i, int flip,
                     hipStream_t st);
// The 3x3x3 stride-1 conv (forward, and input gradient with flipped taps): ONE plan per geometry, made by conv3_s1_plan
// and read by everything that has to agree on it - the launcher, the split-K scratch and statistics-slab queries, the
// slab finalizers and the "can this be fused" predicates.  choice[] is the order of preference; what only the launch
// knows (operand alignment, whether scratch / a slab / a residual was passed) picks among them in conv_mfma_launch.
enum { S1_SLIDE32 = 1, S1_SLIDE64, S1_WS, S1_PC4, S1_PC, S1_SK, S1_TILE };
struct SlidePlan {
    int dsplit, DL, tiles_h, tiles_w, units, grid, ny;
};
struct Conv3S1Choice {
    int family;               // S1_*
    int td, th, tw, mt, nt;   // spatial tile; mt / nt: 32-voxel / 32-cout MFMA tiles per wave (tile and pc kernels)
    int ks;                   // split-K slices: ks > 1 (S1_WS: any ks) needs ks x voxels x Cout floats of scratch
    char name[40];            // what the launch log reports (the sliding kernels append their epilogue form)
};
struct Conv3S1Plan {
    int count = 0;            // 0: not a 3x3x3 stride-1 gather with Cin, Cout multiples of 32 (the direct kernels' form)
    Conv3S1Choice choice[5];
    SlidePlan slide;          // choice[0] is a sliding kernel: its decomposition
    int pc_gx = 0, pc_gy = 0; // persistent grid of the producer/consumer choice
    size_t ws_bytes = 0;      // split-K scratch a launch can use (without it the next choice runs)
    // fused forms.  can_stats: the first choice sums InstanceNorm statistics into a slab[(y * gx + workgroup) * 4 + wave]
    // [n][cb][2]; can_bwd_sums / can_partner: it is the 32-channel sliding kernel (backward sums, 1x1x1 partner as a 28th tap)
    bool can_stats = false, can_bwd_sums = false, can_partner = false;
    int gx = 0, gy = 0, cb = 0;
    size_t slab_bytes = 0;
};
Conv3S1Plan conv3_s1_plan(const ConvGeom& g);
// plan: conv3_s1_plan(g) when the caller has it already (NULL: made here)
int conv_mfma_launch(const void* x, const void* w, const float* bias, const void* res, void* y, const ConvGeom& g,
                     hipStream_t st, float* stat_slab = nullptr, void* ws = nullptr, size_t ws_bytes = 0,
                     const void* bst_act = nullptr, int bst_ld = 0, float slope = 0.f, const void* x2 = nullptr,
                     int ldx2 = 0, const void* w2 = nullptr, int* defer_ks = nullptr, const Conv3S1Plan* plan = nullptr);
// slab[(y * gx + workgroup) * 4 + wave][n][cb][2] of per-wave (sum, sum of squares) -> mean / scale (or, scale == NULL,
// the two means m12[n][c] = (mean g', mean g' xhat) of the backward sums)
int stats_slab_finalize_launch(const float* slab, int gx, int cb, int N, int C, double invV, const float* drop, float eps,
                               float* mean, float* scale, hipStream_t st);
// The weight gradient of every conv form: ONE plan per (geometry, dtype), made by wgrad_plan and read by everything that
// has to agree on it - the launcher, the workspace queries, the pair and bias entry points and the "can this take a split
// x" question.  The families in order of preference; what only the launch knows (operand alignment, the workspace that
// was passed, dw's alignment for the direct store) is checked in wgrad_launch.
enum { WG_STEM_MFMA = 1, WG_STEM, WG_HEAD, WG_SLIDE, WG_S1_TILE, WG_S2, WG_STAGED, WG_GENERIC };
struct WgradSlidePlan {
    int dsplit, DL, tiles_h, tiles_w, units, G, pairs;
};
struct WgradPlan {
    int family = 0;           // WG_*; 0: nothing takes this geometry and dtype (refusal says why)
    const char* refusal = nullptr;
    int groups = 0;           // slabs the main kernel writes = the count handed to wgrad_reduce_launch
    WgradSlidePlan slide = {};   // WG_SLIDE: its decomposition
    int td = 0, th = 0, tw = 0;   // WG_S1_TILE: the halo tile; WG_S2: tw = tile width
    bool direct = false;      // WG_S1_TILE: a lone workgroup per pair and dw in the Conv3d layout - stored without slabs
    int nco = 0;              // WG_S2: 32-cout tiles per workgroup
    bool dma = false;         // WG_S2: the LDS-DMA kernel (else the register-staged one)
    int pt = 0;               // WG_STAGED: positions per tile (the taps are g.taps)
    // What the workspace queries report: an upper BOUND, not what `family` writes.  Callers size pooled buffers from it and
    // the figure predates the plan: max(tile, slide) for the 3x3x3 stride-1 form, max(staged, s2) for the other MFMA forms,
    // the larger of the stem's two kernels (28 rows: the bias row included).  Set for a refused split x too.
    size_t ws_bytes = 0;
    bool can_pair = false;    // the 28-tap pair form (WG_SLIDE / WG_S2 with dma) takes this geometry
    size_t pair_ws_bytes = 0;
    bool gives_bias = false;  // the bias row comes from the same pass (WG_STEM_MFMA)
    char name[40] = "", pair_name[40] = "";   // what the launch log reports (single / pair form)
};
WgradPlan wgrad_plan(const WgradGeom& g, int dtype);
// dy2 / dw2: the pair form (plan.can_pair); db: the bias row (plan.gives_bias)
int wgrad_launch(const WgradPlan& p, const void* x, const void* dy, float* dw, void* ws, size_t ws_bytes,
                 const WgradGeom& g, int dtype, hipStream_t st, const void* dy2 = nullptr, int lddy2 = 0,
                 float* dw2 = nullptr, float* db = nullptr);
bool mfma_wgrad_eligible(const WgradGeom& g, int dtype);

// conv_slide32.hip (3x3x3 stride-1, 32 -> 32 / 64 channels: D-sliding plane ring on v_mfma_f32_16x16x32, a wave = all 32
// couts of a 4 x 16 quarter of the column, the whole weight resident in AGPRs)
bool slide_conv_plan(int N, int D, int H, int W, int Cin, int Cout, SlidePlan* out);
// bst_act != NULL (input-gradient role): the slab receives the InstanceNorm + LeakyReLU backward sums of the output
// against the activation bst_act (pitch bst_ld) instead of the forward statistics
// x2 / ldx2 / w2: a second tensor on the output grid (32 channels) and a packed 1x1x1 input-gradient weight: y += W2^T x2
int conv_slide_launch(const void* x, const void* w, const float* bias, const void* res, void* y, const ConvGeom& g,
                      const SlidePlan& p, float* stat_slab, hipStream_t st, const void* bst_act = nullptr, int bst_ld = 0,
                      float slope = 0.f, const void* x2 = nullptr, int ldx2 = 0, const void* w2 = nullptr);

// conv_slide64.hip (3x3x3 stride-1, 64 -> 64 / 128 channels: the same design on v_mfma_f32_16x16x32, a wave = 16 couts)
// edge: a last column narrower than the tile may run masked
bool slide64_conv_plan(int N, int D, int H, int W, int Cin, int Cout, bool edge, SlidePlan* out);
// whole-sample form of the deepest level (conv_ws.hip): split-K slices for this geometry (0 = not its shape); the kernel
// writes fp32 partials [slice][voxel][Cout] for conv_ksplit_reduce_kernel.  mode 2: wherever the shape fits
int conv_ws_slices(int N, int D, int H, int W, int Cin, int Cout, int mode);
int conv_ws_launch(const void* x, const void* w, float* part, int N, int D, int H, int W, int Cin, int Cout, int ldx,
                   int flip, int slices, hipStream_t st);
int conv_slide64_launch(const void* x, const void* w, const float* bias, const void* res, void* y, const ConvGeom& g,
                        const SlidePlan& p, float* stat_slab, hipStream_t st);

// conv_direct.hip.  The MFMA forms conv3_s1_plan leaves (count == 0): 3x3x3 stride-2 gather, transposed, 1x1x1.  ONE plan
// per geometry, made by conv_direct_plan and read by the launcher, the slab queries and the fused entry points with their
// "supported" predicates.  At most two choices: the LDS-DMA tile kernel of conv_s2.hip where the geometry is eligible
// (tile != 0; what only a launch knows about it is asked of conv_direct_tile_ok, by the launcher and the predicates
// alike), then exactly one fallback without launch-time conditions, its template parameters stored as data.
enum { S2_TILE_T = 1, S2_TILE_G };      // transposed / gather form
enum { DIRECT_KSPLIT = 1, DIRECT_CONVT_TILE, DIRECT_GATHER, DIRECT_T };
struct ConvDirectPlan {
    int tile = 0;             // S2_TILE_*; 0: no tile kernel for this geometry
    SlidePlan slide = {};     // its decomposition
    int tile_tw = 0;          // tile width (T form)
    char tile_name[40] = "";  // what the launch log reports
    // the tile kernel's statistics slab[(y * gx + workgroup) * 4 + wave][n][cb][2].  Set wherever the decomposition exists,
    // for a pitch or an extent the kernel refuses too: the workspace queries report it and predate the plan
    int gx = 0, cb = 0;
    size_t slab_bytes = 0;
    int family = 0;           // DIRECT_*; 0: nothing takes this geometry (refusal says why) and nothing is launched
    const char* refusal = nullptr;
    int nt = 0;               // 32-cout tiles per workgroup
    int rd = 0;               // K-split / gather: prefetch depth
    int td = 0, th = 0, tw = 0;   // DIRECT_CONVT_TILE: the half-resolution tile
    char name[40] = "";
};
ConvDirectPlan conv_direct_plan(const ConvGeom& g);
// may this launch run the plan's tile kernel?  partner: a fused pair's second gradient (T form) / second output (G form)
bool conv_direct_tile_ok(const ConvDirectPlan& p, const ConvGeom& g, const void* x, const void* res, const void* y,
                         const void* partner = nullptr, int ld_partner = 0);
int conv_direct_launch(const ConvDirectPlan& p, const void* x, const void* w, const float* bias, const void* res, void* y,
                       const ConvGeom& g, hipStream_t st);

// conv_s2.hip (the stride-2 forms of the large levels: LDS-DMA plane ring, producer wave, weights in registers): the tile
// halves of conv_direct_plan and the launches that read them back.  x2 / ldx2 / w2 and w2 / bias2 / y2 / ldy2: the fused pairs
bool convt_s2_tile_plan(const ConvGeom& g, ConvDirectPlan* p);
int convt_s2_tile_launch(const ConvDirectPlan& p, const void* x, const void* w, const float* bias, const void* res, void* y,
                         const ConvGeom& g, float* stat_slab, const void* x2, int ldx2, const void* w2, hipStream_t st);
bool conv_s2_tile_plan(const ConvGeom& g, ConvDirectPlan* p);
int conv_s2_tile_launch(const ConvDirectPlan& p, const void* x, const void* w, const float* bias, void* y, const ConvGeom& g,
                        float* stat_slab, const void* w2, const float* bias2, void* y2, int ldy2, hipStream_t st);

// fused_skip.hip (decoder ResBlock tail: 1x1x1 skip conv + InstanceNorm apply + sum + LeakyReLU in one pass)
bool skip1x1_fused_eligible(const ru3d_tensor* x, const ru3d_tensor* y2, const ru3d_tensor* out, int dtype);
// head_w / head_bias / logits: the head-carrying form (the network's 1x1x1 head on the block's output in the same pass)
bool skip1x1_head_fused_eligible(const ru3d_tensor* x, const ru3d_tensor* y2, const ru3d_tensor* out,
                                 const ru3d_tensor* logits, int dtype);
int skip1x1_fused_launch(const ru3d_tensor* x, const void* w, const float* bias, const ru3d_tensor* y2, const float* mean,
                         const float* scale, const ru3d_tensor* out, float slope, hipStream_t st,
                         const void* head_w = nullptr, const float* head_bias = nullptr, const ru3d_tensor* logits = nullptr);

// norm_small.hip (InstanceNorm + LeakyReLU of the small levels).  in_small_mode: 0 = not its shape (norm.hip's three
// launches), 1 = whole-instance kernel (one launch; can sum a conv's split-K slices itself), 2 = two coalesced kernels.
int in_small_mode(const ru3d_tensor* y, bool all_samples, const ru3d_tensor* a = nullptr, const ru3d_tensor* b = nullptr,
                  const ru3d_tensor* c = nullptr, const ru3d_tensor* d = nullptr);
size_t in_small_ws_bytes(const ru3d_tensor* y);
int in_small_fwd_launch(const ru3d_tensor* y, const float* part, int ksplit, const float* bias, const float* drop,
                        float* mean, float* scale, const ru3d_tensor* res, const ru3d_tensor* out, void* ws, float eps,
                        float slope, hipStream_t st);
int in_small_bwd_launch(const ru3d_tensor* gout, const float* part, int ksplit, const ru3d_tensor* outp,
                        const ru3d_tensor* y, const float* mean, const float* scale, const ru3d_tensor* dy,
                        const ru3d_tensor* gpre, void* ws, float slope, int zero_far, float* gpre_sum, hipStream_t st);

// The per-family halves of wgrad_plan and wgrad_launch.  A *_plan fills its part of the plan (decomposition, groups) and
// says whether the family takes the geometry; a *_launch reads it back (dy2 != NULL: the pair form).
// wgrad_slide.hip (3x3x3 stride-1 weight gradient on the large levels: D-sliding plane ring)
bool wgrad_slide_plan(const WgradGeom& g, WgradPlan* p);
int wgrad_slide_launch(const void* x, const void* dy, const void* dy2, int lddy2, float* dw, float* dw2, void* ws,
                       const WgradGeom& g, const WgradPlan& p, hipStream_t st);
// wgrad_s2.hip (3x3x3 stride-2 / ConvTranspose weight gradient on the large levels: one parity-split input tile)
bool wgrad_s2_plan(const WgradGeom& g, WgradPlan* p);
int wgrad_s2_launch(const void* x, const void* dy, const void* dy2, int lddy2, float* dw, float* dw2, void* ws,
                    const WgradGeom& g, const WgradPlan& p, hipStream_t st);

// small_convs.hip (1-channel stem, 2..4-channel head)
bool stem_fwd_eligible(const ConvGeom& g, int dtype, int y_dtype, const void* res);
int stem_fwd_launch(const void* x, const void* w, const float* bias, void* y, const ConvGeom& g, int dtype,
                    hipStream_t st);
bool head_fwd_eligible(const ConvGeom& g, int dtype, const void* res);
int head_fwd_launch(const void* x, const void* w, const float* bias, void* y, const ConvGeom& g, int dtype,
                    int y_dtype, hipStream_t st);
bool head_dgrad_eligible(const ConvGeom& g, int dtype, int y_dtype, const void* res);
int head_dgrad_launch(const void* dy, const void* w, void* dx, const ConvGeom& g, int dtype, hipStream_t st);
bool stem_wgrad_plan(const WgradGeom& g, int dtype, WgradPlan* p);
int stem_wgrad_launch(const void* x, const void* dy, float* dw, float* db, void* ws, const WgradGeom& g,
                      const WgradPlan& p, int dtype, hipStream_t st);
// the head's whole backward in one pass over (a, dlogits fp32): dx, dW, db
bool head_bwd_eligible(int Cin, int Cout, int dtype);
size_t head_bwd_ws_bytes(int64_t P, int Cin);
int head_bwd_launch(const void* a, int lda, const float* dlog, int ldd, const float* w, int cin_real, int Cin, int Cout,
                    void* dx, int lddx, float* dw, float* db, void* ws, int64_t P, hipStream_t st);
// (dx == NULL: dW and db alone - head_bwd_wgrad_kernel, same sums)
bool head_wgrad_plan(const WgradGeom& g, int dtype, WgradPlan* p);
int head_wgrad_launch(const void* x, const void* dy, float* dw, void* ws, const WgradGeom& g, const WgradPlan& p,
                      int dtype, hipStream_t st);

}  // namespace RU3D_NS
using namespace RU3D_NS;
