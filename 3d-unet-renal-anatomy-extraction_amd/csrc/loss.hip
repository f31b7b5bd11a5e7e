// Fused softmax + focal + Tversky loss (forward sums, on-device finalize, backward) and the functional Tversky `dice`.
// One read of logits + labels per pass; per-thread fp32 partials -> wave shuffles -> LDS -> one double partial per
// block -> fixed-order finalize (deterministic, no atomics, no host sync).  The arithmetic itself is loss_core.h's,
// shared with deepsup.hip; this file holds the single-tensor kernels and their entry points.
//
// Reference arithmetic restated (loss.py): with p = softmax(z) (sigmoid when C == 1), g = one_hot(t):
//   tp_c = sum p_c g_c, fn_c = sum (1-p_c) g_c = sg_c - tp_c, fp_c = sum p_c (1-g_c) = sp_c - tp_c
//   dice_c  = (tp_c + s) / (tp_c + alpha fn_c + beta fp_c + s)                      loss.py:32-48
//   focal_c = C * mean_v( -(1-p_c)^gamma g_c log p_c )                              loss.py:78-79, 240-241
//   w       = weight_v / |weight_v|_1   (weight_c and the presence mask are dead)   loss.py:69,155,237
//   Hybird  = sum_c w_c (1 - dice_c + focal_c); DiceLoss = sum w (1 - dice); Focal = sum w focal;
//   Dice    = sum w dice
// With an ignore label (the IGN instantiations, ru3d_loss_ignore_fwd / _bwd) all of this is taken over the voxels whose
// label is not the ignore label, M of them: tp, sp, sg over those only, focal_c = C * sum / max(M, 1) with M = sum_c sg_c,
// and exact zeros written as the gradient of the others, whose logits are never read.
#include "common.h"
#include "loss_core.h"

struct LossState {
    RegionCoef r;
    int pad[2];
};

extern "C" size_t ru3d_loss_state_bytes(int num_classes) {
    (void)num_classes;
    return sizeof(LossState);
}

extern "C" size_t ru3d_loss_state_bad_labels_offset(void) { return offsetof(LossState, r) + offsetof(RegionCoef, bad_labels); }

extern "C" size_t ru3d_loss_workspace_bytes(int n, int64_t v, int num_classes) {
    (void)num_classes;
    return (size_t)region_fwd_blocks((int64_t)n * v) * REGION_Q * sizeof(double);
}

template <int C, bool IGN>
__global__ __launch_bounds__(256) void loss_sums_kernel(const float* __restrict__ logits, int64_t stride_n,
                                                        int64_t stride_c, int64_t stride_v,
                                                        const void* __restrict__ labels, int label_dtype, int n,
                                                        int64_t v, float gamma, int ignore_label,
                                                        double* __restrict__ part) {
    float tp[C], sp[C], sg[C], fo[C];
#pragma unroll
    for (int c = 0; c < C; c++) tp[c] = sp[c] = sg[c] = fo[c] = 0.f;
    int bad = 0;
    const int64_t total = (int64_t)n * v;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const int64_t ni = i / v, vi = i - ni * v;
        const int t = load_label(labels, label_dtype, i);
        if (label_ignored<IGN>(t, ignore_label)) continue;
        float p[C], lp[C];
        voxel_probs<C>(logits + ni * stride_n + vi * stride_v, stride_c, p, lp);
        region_add<C>(p, lp, t, gamma, tp, sp, sg, fo, bad);
    }
    region_write_row<C>(tp, sp, sg, fo, bad, part + (int64_t)blockIdx.x * REGION_Q);
}

struct LossParams {
    int kind, C, n;
    int64_t v;
    float gamma, alpha, beta, smooth;
    float w[RU3D_MAX_CLASSES];  // weight_v (un-normalised); all ones when the caller passed NULL
};

template <bool IGN>
__global__ __launch_bounds__(REGION_LF_THREADS) void loss_finalize_kernel(const double* __restrict__ part, int blocks,
                                                                          LossParams P, LossState* __restrict__ st,
                                                                          float* __restrict__ loss_out) {
    __shared__ double red[REGION_LF_GROUPS][REGION_Q];
    __shared__ double tot[REGION_Q];
    region_reduce_rows(part, blocks, P.C, red, tot);
    if (threadIdx.x != 0) return;
    const double nv = region_voxels<IGN>((double)P.n * (double)P.v, P.C, tot);
    loss_out[0] = (float)region_coefficients(P.kind, P.C, P.w, P.alpha, P.beta, P.smooth, nv, tot,
                                             (int)tot[4 * RU3D_MAX_CLASSES], &st->r);
}

template <int C, typename TG, bool IGN>
__global__ __launch_bounds__(256) void loss_bwd_kernel(const float* __restrict__ logits, int64_t stride_n,
                                                       int64_t stride_c, int64_t stride_v,
                                                       const void* __restrict__ labels, int label_dtype, int n,
                                                       int64_t v, float gamma, int ignore_label,
                                                       const LossState* __restrict__ st,
                                                       const float* __restrict__ grad_out, TG* __restrict__ dz) {
    const RegionGrad<C> grad(&st->r);
    const float go = grad_out ? grad_out[0] : 1.f;
    const int64_t total = (int64_t)n * v;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const int64_t ni = i / v, vi = i - ni * v;
        const int64_t base = ni * stride_n + vi * stride_v;
        const int t = load_label(labels, label_dtype, i);
        if (label_ignored<IGN>(t, ignore_label)) {      // dz is uninitialised memory: the zeros are written
#pragma unroll
            for (int c = 0; c < C; c++) dz[base + c * stride_c] = from_f32<TG>(0.f);
            continue;
        }
        float p[C], lp[C], d[C];
        voxel_probs<C>(logits + base, stride_c, p, lp);
        grad.voxel(p, lp, t, gamma, d);
#pragma unroll
        for (int c = 0; c < C; c++) dz[base + c * stride_c] = from_f32<TG>(d[c] * go);
    }
}

extern "C" int ru3d_loss_ignore_fwd(const float* logits, int64_t stride_n, int64_t stride_c, int64_t stride_v,
                                    const void* labels, int label_dtype, int n, int64_t v, int num_classes,
                                    int has_ignore, int ignore_label, int kind, float gamma, const float* weight_v,
                                    float alpha, float beta, float smooth, void* state, float* loss_out, void* ws,
                                    size_t ws_bytes, void* stream) {
    Ru3dDeviceGuard dev_guard(stream);
    int rc = loss_view_check("loss_fwd", logits && labels && state && loss_out && ws, n > 0 && v > 0, label_dtype,
                             num_classes, 1);
    if (rc) return rc;
    rc = loss_ignore_check("loss_fwd", has_ignore, ignore_label, label_dtype, num_classes);
    if (rc) return rc;
    RU3D_REQUIRE(kind >= 0 && kind <= 3, "loss_fwd: bad kind %d", kind);
    RU3D_REQUIRE(ws_bytes >= ru3d_loss_workspace_bytes(n, v, num_classes), "loss_fwd: workspace too small");
    hipStream_t st = as_stream(stream);
    const int blocks = region_fwd_blocks((int64_t)n * v);
#define CALL(CC, IGN)                                                                                          \
    hipLaunchKernelGGL((loss_sums_kernel<CC, IGN>), dim3(blocks), dim3(256), 0, st, logits, stride_n, stride_c, \
                       stride_v, labels, label_dtype, n, v, gamma, ignore_label, (double*)ws)
    RU3D_DISPATCH_C_IGN(1, num_classes, has_ignore, CALL)
#undef CALL
    rc = ru3d_check_launch("loss_sums");
    if (rc) return rc;
    LossParams P;
    P.kind = kind;
    P.C = num_classes;
    P.n = n;
    P.v = v;
    P.gamma = gamma;
    P.alpha = alpha;
    P.beta = beta;
    P.smooth = smooth;
    fill_class_weights(P.w, weight_v, num_classes);
    if (has_ignore)
        hipLaunchKernelGGL(loss_finalize_kernel<true>, dim3(1), dim3(REGION_LF_THREADS), 0, st, (const double*)ws, blocks,
                           P, (LossState*)state, loss_out);
    else
        hipLaunchKernelGGL(loss_finalize_kernel<false>, dim3(1), dim3(REGION_LF_THREADS), 0, st, (const double*)ws, blocks,
                           P, (LossState*)state, loss_out);
    return ru3d_check_launch("loss_finalize");
}

extern "C" int ru3d_loss_fwd(const float* logits, int64_t stride_n, int64_t stride_c, int64_t stride_v,
                             const void* labels, int label_dtype, int n, int64_t v, int num_classes, int kind,
                             float gamma, const float* weight_v, float alpha, float beta, float smooth, void* state,
                             float* loss_out, void* ws, size_t ws_bytes, void* stream) {
    return ru3d_loss_ignore_fwd(logits, stride_n, stride_c, stride_v, labels, label_dtype, n, v, num_classes, 0, 0, kind,
                                gamma, weight_v, alpha, beta, smooth, state, loss_out, ws, ws_bytes, stream);
}

extern "C" int ru3d_loss_ignore_bwd(const float* logits, int64_t stride_n, int64_t stride_c, int64_t stride_v,
                                    const void* labels, int label_dtype, int n, int64_t v, int num_classes,
                                    int has_ignore, int ignore_label, float gamma, const void* state,
                                    const float* grad_out, void* dlogits, int dlogits_dtype, void* stream) {
    Ru3dDeviceGuard dev_guard(stream);
    int rc = loss_view_check("loss_bwd", logits && labels && state && dlogits, n > 0 && v > 0, label_dtype, num_classes, 1);
    if (rc) return rc;
    rc = loss_ignore_check("loss_bwd", has_ignore, ignore_label, label_dtype, num_classes);
    if (rc) return rc;
    RU3D_REQUIRE(dlogits_dtype == RU3D_F32 || dlogits_dtype == RU3D_BF16, "loss_bwd: bad dlogits dtype");
    hipStream_t st = as_stream(stream);
    const int blocks = flat_bwd_blocks((int64_t)n * v, 8192);
#define CALL(CC, TG, IGN)                                                                                        \
    hipLaunchKernelGGL((loss_bwd_kernel<CC, TG, IGN>), dim3(blocks), dim3(256), 0, st, logits, stride_n, stride_c, \
                       stride_v, labels, label_dtype, n, v, gamma, ignore_label, (const LossState*)state, grad_out,  \
                       (TG*)dlogits)
    RU3D_DISPATCH_C_DZ_IGN(1, num_classes, dlogits_dtype, has_ignore, CALL)
#undef CALL
    return ru3d_check_launch("loss_bwd");
}

extern "C" int ru3d_loss_bwd(const float* logits, int64_t stride_n, int64_t stride_c, int64_t stride_v,
                             const void* labels, int label_dtype, int n, int64_t v, int num_classes, float gamma,
                             const void* state, const float* grad_out, void* dlogits, int dlogits_dtype,
                             void* stream) {
    return ru3d_loss_ignore_bwd(logits, stride_n, stride_c, stride_v, labels, label_dtype, n, v, num_classes, 0, 0, gamma,
                                state, grad_out, dlogits, dlogits_dtype, stream);
}

// --------------------------------------------------------------------------- functional dice
__global__ __launch_bounds__(256) void tversky_sums_kernel(const float* __restrict__ p, const float* __restrict__ g,
                                                           int64_t count, double* __restrict__ part) {
    float tp = 0.f, sp = 0.f, sg = 0.f;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < count; i += (int64_t)gridDim.x * 256) {
        const float a = p[i], b = g[i];
        tp = fmaf(a, b, tp);
        sp += a;
        sg += b;
    }
    __shared__ double sh[4][3];
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    const float a = wave_sum(tp), b = wave_sum(sp), c = wave_sum(sg);
    if (lane == 0) {
        sh[wid][0] = a;
        sh[wid][1] = b;
        sh[wid][2] = c;
    }
    __syncthreads();
    if (threadIdx.x < 3)
        part[(int64_t)blockIdx.x * 3 + threadIdx.x] =
            sh[0][threadIdx.x] + sh[1][threadIdx.x] + sh[2][threadIdx.x] + sh[3][threadIdx.x];
}

__global__ void tversky_finalize_kernel(const double* __restrict__ part, int blocks, float alpha, float beta,
                                        float smooth, float* __restrict__ out) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    double tp = 0.0, sp = 0.0, sg = 0.0;
    for (int b = 0; b < blocks; b++) {
        tp += part[b * 3];
        sp += part[b * 3 + 1];
        sg += part[b * 3 + 2];
    }
    out[0] = (float)((tp + smooth) / (tp + alpha * (sg - tp) + beta * (sp - tp) + smooth));
}

extern "C" int ru3d_tversky(const float* p, const float* g, int64_t count, float alpha, float beta, float smooth,
                            float* out, void* ws, size_t ws_bytes, void* stream) {
    Ru3dDeviceGuard dev_guard(stream);
    RU3D_REQUIRE(p && g && out && ws && count > 0, "tversky: bad argument");
    int blocks = (int)((count + 2047) / 2048);
    if (blocks > 1024) blocks = 1024;
    RU3D_REQUIRE(ws_bytes >= (size_t)blocks * 3 * sizeof(double), "tversky: workspace too small");
    hipLaunchKernelGGL(tversky_sums_kernel, dim3(blocks), dim3(256), 0, as_stream(stream), p, g, count, (double*)ws);
    int rc = ru3d_check_launch("tversky_sums");
    if (rc) return rc;
    hipLaunchKernelGGL(tversky_finalize_kernel, dim3(1), dim3(64), 0, as_stream(stream), (const double*)ws, blocks,
                       alpha, beta, smooth, out);
    return ru3d_check_launch("tversky_finalize");
}
