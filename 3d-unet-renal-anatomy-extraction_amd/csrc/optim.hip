// The optimisers and what surrounds them: fused Adam (single tensor, multi-tensor, captured, and under the on-device fp16
// loss scaler), the global L2 norm of the gradients with the clipping coefficient of torch.nn.utils.clip_grad_norm_, SGD
// with (Nesterov) momentum and weight decay, AdamW, Adam with a clipped gradient, and the inf / nan check of loss scaling.
// Every multi-tensor kernel takes its share of the ru3d_adam_tensor table from table_chunk(), the one place that reads
// the (tensor, chunk) block map of ru3d_adam_multi, and walks it with one of two loops: multi_body (parameter, gradient
// and state: every update rule) or grad_walk (the gradient alone: check, norm, scaling).  Both: 256 threads, chunk_elems
// a multiple of 1024, an aligned f32x4 path and a scalar path for tails and for tensors that do not sit on 16-byte
// boundaries, rows with a null `grad` skipped.
//
// Bits: each update rule is ONE per-element function compiled with floating-point contraction off, called from the
// vector path and from the scalar path, by the kernel that takes its scalars as arguments and by the one that reads
// them from the 8-float device row of a captured step - the four give identical bits (AdamRule's lesson, below).  A
// clipped and an unclipped step share a kernel: the coefficient is 1 without one, and x * 1.0f is x.  No
// floating-point atomics: the norm is a float64 sum of float64 squares, thread -> wave butterfly -> the four waves of a
// block in order -> one workgroup over the per-block partials in order.
#include "common.h"
#include <stddef.h>

// --------------------------------------------------------------------------- the table walk
// A block's share of the table: its row and the elements [begin, end) of that row's tensors.  A thread takes the 4-wide
// slots at begin + 4 * threadIdx.x, + kSlotStride, ... in ascending order, and k = 0..3 inside a slot.
struct TableChunk {
    ru3d_adam_tensor t;
    int64_t begin, end;
};
static constexpr int kSlotStride = 1024;        // 256 threads x 4 elements; chunk_elems is a multiple of it

__device__ __forceinline__ TableChunk table_chunk(const ru3d_adam_tensor* __restrict__ tensors,
                                                  const int32_t* __restrict__ block_map, int chunk_elems) {
    TableChunk c;
    c.t = tensors[block_map[2 * blockIdx.x]];
    c.begin = (int64_t)block_map[2 * blockIdx.x + 1] * chunk_elems;
    c.end = c.begin + chunk_elems;
    if (c.end > c.t.count) c.end = c.t.count;
    return c;
}

// The update walk.  rule.first(): the rule keeps a first buffer in `exp_avg` (momentum / first moment); Rule::kSecond: it
// keeps `exp_avg_sq`.  coef: the device-side clipping coefficient, null for an unclipped step.
template <class Rule>
__device__ __forceinline__ void multi_body(const ru3d_adam_tensor* __restrict__ tensors,
                                           const int32_t* __restrict__ block_map, int chunk_elems, const Rule rule,
                                           const float* __restrict__ coef) {
    const TableChunk ch = table_chunk(tensors, block_map, chunk_elems);
    const ru3d_adam_tensor& t = ch.t;
    if (!t.grad) return;
    const bool first = rule.first();
    if ((first && !t.exp_avg) || (Rule::kSecond && !t.exp_avg_sq)) return;      // a row without its state is left alone
    const int64_t end = ch.end;
    const float c = coef ? *coef : 1.f;          // x * 1.0f is x: the unclipped step needs no second body
    uintptr_t bits = ((uintptr_t)t.param) | ((uintptr_t)t.grad);
    if (first) bits |= (uintptr_t)t.exp_avg;
    if (Rule::kSecond) bits |= (uintptr_t)t.exp_avg_sq;
    int64_t i = ch.begin + (int64_t)threadIdx.x * 4;
    if ((bits & 15) == 0) {
        for (; i + 3 < end; i += kSlotStride) {
            f32x4 p = *reinterpret_cast<const f32x4*>(t.param + i);
            const f32x4 g = *reinterpret_cast<const f32x4*>(t.grad + i);
            f32x4 m = {0.f, 0.f, 0.f, 0.f}, v = {0.f, 0.f, 0.f, 0.f};
            if (first) m = *reinterpret_cast<const f32x4*>(t.exp_avg + i);
            if (Rule::kSecond) v = *reinterpret_cast<const f32x4*>(t.exp_avg_sq + i);
#pragma unroll
            for (int k = 0; k < 4; k++) {
                float pk = p[k], mk = m[k], vk = v[k];
                rule.elem(pk, g[k], c, mk, vk);
                p[k] = pk; m[k] = mk; v[k] = vk;
            }
            *reinterpret_cast<f32x4*>(t.param + i) = p;
            if (first) *reinterpret_cast<f32x4*>(t.exp_avg + i) = m;
            if (Rule::kSecond) *reinterpret_cast<f32x4*>(t.exp_avg_sq + i) = v;
        }
    }
    // scalar tail (or unaligned tensors): this thread's remaining elements of its 4-wide slots
    for (; i < end; i += kSlotStride)
        for (int k = 0; k < 4 && i + k < end; k++) {
            float pk = t.param[i + k], mk = first ? t.exp_avg[i + k] : 0.f, vk = Rule::kSecond ? t.exp_avg_sq[i + k] : 0.f;
            rule.elem(pk, t.grad[i + k], c, mk, vk);
            t.param[i + k] = pk;
            if (first) t.exp_avg[i + k] = mk;
            if (Rule::kSecond) t.exp_avg_sq[i + k] = vk;
        }
}

// The gradient-only walk: every element g[j] of the chunk is loaded, handed to op, and - when `write` - replaced by
// what op returned.  Nothing else is loaded or stored.  The caller has checked that the row has a gradient.
template <class Op>
__device__ __forceinline__ void grad_walk(const TableChunk& ch, bool write, Op op) {
    float* g = const_cast<float*>(ch.t.grad);
    const int64_t end = ch.end;
    int64_t i = ch.begin + (int64_t)threadIdx.x * 4;
    if ((((uintptr_t)g) & 15) == 0) {
        for (; i + 3 < end; i += kSlotStride) {
            f32x4 v = *reinterpret_cast<const f32x4*>(g + i);
#pragma unroll
            for (int k = 0; k < 4; k++) v[k] = op(v[k]);
            if (write) *reinterpret_cast<f32x4*>(g + i) = v;
        }
    }
    for (; i < end; i += kSlotStride)
        for (int k = 0; k < 4 && i + k < end; k++) {
            const float v = op(g[i + k]);
            if (write) g[i + k] = v;
        }
}

// --------------------------------------------------------------------------- SGD
// torch.optim.SGD with dampening = 0, maximize = False:  gh = g * gscale * coef;  d = gh + wd * p;
// b = mu * b + d (mu != 0; a zero buffer makes the first step torch's b = d);  u = nesterov ? d + mu * b : b  (u = d
// when mu == 0);  p -= lr * u.  The momentum buffer travels in the `exp_avg` slot.
struct SgdRule {
    float lr, mu, wd, gscale;
    bool nesterov;
    static constexpr bool kSecond = false;
    __device__ __forceinline__ bool first() const { return mu != 0.f; }
    __device__ __forceinline__ void elem(float& p, float g, float c, float& b, float&) const {
#pragma clang fp contract(off)
        const float gh = g * gscale * c;
        float d = gh;
        if (wd != 0.f) d = gh + wd * p;
        float u = d;
        if (mu != 0.f) {
            b = mu * b + d;
            u = nesterov ? d + mu * b : b;
        }
        p -= lr * u;
    }
};

// hyper row of a captured SGD step: {lr, momentum, weight_decay, nesterov (0 / 1), -, -, grad_scale, -}
__device__ __forceinline__ SgdRule sgd_rule(float lr, float mu, float wd, float nesterov, float gscale) {
    SgdRule r;
    r.lr = lr; r.mu = mu; r.wd = wd; r.gscale = gscale; r.nesterov = nesterov != 0.f;
    return r;
}

__global__ __launch_bounds__(256) void sgd_multi_kernel(const ru3d_adam_tensor* __restrict__ tensors,
                                                        const int32_t* __restrict__ block_map, int chunk_elems, float lr,
                                                        float mu, float wd, float nesterov, float gscale,
                                                        const float* __restrict__ coef) {
    multi_body(tensors, block_map, chunk_elems, sgd_rule(lr, mu, wd, nesterov, gscale), coef);
}

__global__ __launch_bounds__(256) void sgd_multi_dev_kernel(const ru3d_adam_tensor* __restrict__ tensors,
                                                            const int32_t* __restrict__ block_map, int chunk_elems,
                                                            const float* __restrict__ hyper,
                                                            const float* __restrict__ coef) {
    multi_body(tensors, block_map, chunk_elems, sgd_rule(hyper[0], hyper[1], hyper[2], hyper[3], hyper[6]), coef);
}

// --------------------------------------------------------------------------- Adam and AdamW
// torch.optim.Adam on gh = g * gscale * coef:  m = b1 * m + (1 - b1) * gh;  v = b2 * v + (1 - b2) * gh * gh;
// p -= lr / bc1 * m / (sqrt(v) / sqrt(bc2) + eps).  kDecay: torch.optim.AdamW's p *= 1 - lr * wd first.
// No fused multiply-adds here: the rule is compiled into several kernels (scalars as arguments / from device memory) and
// into a vector and a scalar path - left to the compiler, the contraction of b2 * v + (1 - b2) * g * g differed
// between them by one ulp, on the one parameter whose length is not a multiple of 4 (the head's bias).
template <bool kDecay>
struct AdamRule {
    float b1, b2, eps, step, bc2_sqrt, gscale, keep;
    static constexpr bool kSecond = true;
    __device__ __forceinline__ bool first() const { return true; }
    __device__ __forceinline__ void elem(float& p, float g, float c, float& m, float& v) const {
#pragma clang fp contract(off)
        const float gi = g * gscale * c;
        if (kDecay) p = p * keep;
        m = b1 * m + (1.f - b1) * gi;
        v = b2 * v + (1.f - b2) * gi * gi;
        p -= step * (m / (sqrtf(v) / bc2_sqrt + eps));
    }
};

template <bool kDecay>
__device__ __forceinline__ AdamRule<kDecay> adam_rule(float lr, float b1, float b2, float eps, float bc1, float bc2_sqrt,
                                                      float gscale, float wd) {
#pragma clang fp contract(off)
    AdamRule<kDecay> r;
    r.b1 = b1; r.b2 = b2; r.eps = eps; r.bc2_sqrt = bc2_sqrt; r.gscale = gscale;
    r.step = lr / bc1;
    r.keep = 1.f - lr * wd;
    return r;
}

// Adam, clipped or not: one launch for the whole model.  The scalars of ru3d_adam_multi (sqrt(bias_corr2) taken on the
// host) ...
__global__ __launch_bounds__(256) void adam_multi_kernel(const ru3d_adam_tensor* __restrict__ tensors,
                                                         const int32_t* __restrict__ block_map, int chunk_elems,
                                                         float lr, float b1, float b2, float eps, float bc1,
                                                         float bc2_sqrt, float gscale, const float* __restrict__ coef) {
    multi_body(tensors, block_map, chunk_elems, adam_rule<false>(lr, b1, b2, eps, bc1, bc2_sqrt, gscale, 0.f), coef);
}

// ... or the same scalars from its hyper row in device memory (a captured launch: see ru3d.h)
__global__ __launch_bounds__(256) void adam_multi_dev_kernel(const ru3d_adam_tensor* __restrict__ tensors,
                                                             const int32_t* __restrict__ block_map, int chunk_elems,
                                                             const float* __restrict__ hyper,
                                                             const float* __restrict__ coef) {
    multi_body(tensors, block_map, chunk_elems,
               adam_rule<false>(hyper[0], hyper[1], hyper[2], hyper[3], hyper[4], hyper[7], hyper[6], 0.f), coef);
}

// AdamW: hyper row {lr, beta1, beta2, eps, bias_corr1, bias_corr2, grad_scale, weight_decay} - slot 7 carries the decay,
// so BOTH forms take sqrtf(bias_corr2) here, on the device
__global__ __launch_bounds__(256) void adamw_multi_kernel(const ru3d_adam_tensor* __restrict__ tensors,
                                                          const int32_t* __restrict__ block_map, int chunk_elems, float lr,
                                                          float b1, float b2, float eps, float wd, float bc1, float bc2,
                                                          float gscale, const float* __restrict__ coef) {
    multi_body(tensors, block_map, chunk_elems, adam_rule<true>(lr, b1, b2, eps, bc1, sqrtf(bc2), gscale, wd), coef);
}

__global__ __launch_bounds__(256) void adamw_multi_dev_kernel(const ru3d_adam_tensor* __restrict__ tensors,
                                                              const int32_t* __restrict__ block_map, int chunk_elems,
                                                              const float* __restrict__ hyper,
                                                              const float* __restrict__ coef) {
    multi_body(tensors, block_map, chunk_elems,
               adam_rule<true>(hyper[0], hyper[1], hyper[2], hyper[3], hyper[4], sqrtf(hyper[5]), hyper[6], hyper[7]),
               coef);
}

// ---- fp16 training inside a captured step: the loss scaler lives on the device (ru3d_amp_state, see ru3d.h).  The update
// kernel skips itself when the gradient check found an overflow, takes 1 / scale and the number of steps really taken
// from the state block (bias corrections from that count), and a one-thread kernel then moves the scaler: halve + reset
// on overflow, count a clean step and double after `growth_interval` of them otherwise - apex's schedule
// (reference trainer.py:492-493, 538-542), without the per-step read-back that kept the fp16 step out of a hipGraph.
__global__ __launch_bounds__(256) void adam_multi_amp_kernel(const ru3d_adam_tensor* __restrict__ tensors,
                                                             const int32_t* __restrict__ block_map, int chunk_elems,
                                                             const float* __restrict__ hyper,
                                                             const ru3d_amp_state* __restrict__ amp) {
    if (amp->found_inf != 0.f) return;                                   // overflow: the step is skipped
    const int t = __float_as_int(hyper[5]) + amp->steps + 1;             // Adam step number of this update
    // the betas in double (float value + residual in the slots the captured amp launch does not use otherwise): the bias
    // corrections then equal the host's `1 - beta ** t` to the last bit or two
    const double b1d = (double)hyper[1] + (double)hyper[4], b2d = (double)hyper[2] + (double)hyper[7];
    const double bc1 = 1.0 - pow(b1d, (double)t), bc2 = 1.0 - pow(b2d, (double)t);
    multi_body(tensors, block_map, chunk_elems,
               adam_rule<false>(hyper[0], hyper[1], hyper[2], hyper[3], (float)bc1, sqrtf((float)bc2), amp->inv_scale, 0.f),
               nullptr);
}

__global__ void amp_update_kernel(ru3d_amp_state* amp, float growth, float backoff, int interval, float min_scale,
                                  float max_scale) {
    if (threadIdx.x || blockIdx.x) return;
    if (amp->found_inf != 0.f) {
        amp->scale = fmaxf(amp->scale * backoff, min_scale);
        amp->tracker = 0;
        amp->skipped += 1;
    } else {
        amp->steps += 1;
        amp->tracker += 1;
        if (amp->tracker >= interval) {
            amp->scale = fminf(amp->scale * growth, max_scale);
            amp->tracker = 0;
        }
    }
    amp->inv_scale = 1.f / amp->scale;
    amp->found_inf = 0.f;
}

extern "C" int ru3d_amp_update(ru3d_amp_state* amp, float growth_factor, float backoff_factor, int growth_interval,
                               float min_scale, float max_scale, void* stream) {
    Ru3dDeviceGuard dev_guard(stream);
    RU3D_REQUIRE(amp && growth_factor >= 1.f && backoff_factor > 0.f && backoff_factor <= 1.f && growth_interval > 0 &&
                     min_scale > 0.f && max_scale >= min_scale, "amp_update: bad argument");
    hipLaunchKernelGGL(amp_update_kernel, dim3(1), dim3(64), 0, as_stream(stream), amp, growth_factor, backoff_factor,
                       growth_interval, min_scale, max_scale);
    return ru3d_check_launch("amp_update");
}

// --------------------------------------------------------------------------- Adam: single tensor
__global__ __launch_bounds__(256) void adam_kernel(float* __restrict__ p, const float* __restrict__ g,
                                                   float* __restrict__ m, float* __restrict__ v, int64_t count,
                                                   float lr, float b1, float b2, float eps, float bc1, float bc2_sqrt,
                                                   float gscale) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < count; i += (int64_t)gridDim.x * 256) {
        const float gi = g[i] * gscale;
        const float mi = b1 * m[i] + (1.f - b1) * gi;
        const float vi = b2 * v[i] + (1.f - b2) * gi * gi;
        m[i] = mi;
        v[i] = vi;
        // torch.optim.Adam: denom = sqrt(v)/sqrt(bc2) + eps; p -= lr/bc1 * m/denom
        const float denom = sqrtf(vi) / bc2_sqrt + eps;
        p[i] -= (lr / bc1) * (mi / denom);
    }
}

extern "C" int ru3d_adam_step(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, int64_t count,
                              float lr, float beta1, float beta2, float eps, float bias_corr1, float bias_corr2,
                              float grad_scale, void* stream) {
    Ru3dDeviceGuard dev_guard(stream);
    RU3D_REQUIRE(param && grad && exp_avg && exp_avg_sq && count > 0, "adam_step: bad argument");
    int64_t b = (count + 1023) / 1024;
    if (b > 4096) b = 4096;
    hipLaunchKernelGGL(adam_kernel, dim3((unsigned)b), dim3(256), 0, as_stream(stream), param, grad, exp_avg,
                       exp_avg_sq, count, lr, beta1, beta2, eps, bias_corr1, sqrtf(bias_corr2), grad_scale);
    return ru3d_check_launch("adam_step");
}

// --------------------------------------------------------------------------- loss scaling (fp16 storage)
// Dynamic loss scaling of the reference's mixed-precision mode (apex O1, trainer.py:492-493, 538-542): gradients are
// computed on `scale * loss`; before the optimizer step every gradient is checked for inf / nan (an overflow skips the
// step and halves the scale) and multiplied by 1 / scale.  Same table / block-map layout as ru3d_adam_multi; only the
// `grad` and `count` fields are read.  scale == 1 checks without writing.
__global__ __launch_bounds__(256) void grad_scale_check_kernel(const ru3d_adam_tensor* __restrict__ tensors,
                                                               const int32_t* __restrict__ block_map, int chunk_elems,
                                                               float scale, float* __restrict__ found_inf) {
    const TableChunk ch = table_chunk(tensors, block_map, chunk_elems);
    if (!ch.t.grad) return;
    bool bad = false;
    grad_walk(ch, scale != 1.f, [&](float v) {
        bad = bad || !(fabsf(v) <= 3.402823466e38f);   // false for inf and nan
        return v * scale;
    });
    if (__any(bad) && (threadIdx.x & 63) == 0) *found_inf = 1.f;   // every writer stores the same value
}

// --------------------------------------------------------------------------- gradient norm
// the sum of a block's 256 doubles in a fixed order: butterfly inside each wave (every lane ends with the same bits),
// then wave 0 + wave 1 + wave 2 + wave 3
__device__ __forceinline__ double block_sum_d(double v, double* lds) {
    v = wave_sum_d(v);
    if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = v;
    __syncthreads();
    return ((lds[0] + lds[1]) + lds[2]) + lds[3];
}

// pass 1: partials[block] = sum of the float64 squares of the block's chunk (0 for a row without a gradient).  A thread
// adds its elements in ascending order in both paths, so the alignment of a gradient does not change the sum.
__global__ __launch_bounds__(256) void grad_sumsq_kernel(const ru3d_adam_tensor* __restrict__ tensors,
                                                         const int32_t* __restrict__ block_map, int chunk_elems,
                                                         double* __restrict__ partials) {
    __shared__ double lds[4];
    const TableChunk ch = table_chunk(tensors, block_map, chunk_elems);
    double acc = 0.0;
    if (ch.t.grad)
        grad_walk(ch, false, [&](float v) {
            acc += (double)v * (double)v;
            return v;
        });
    const double s = block_sum_d(acc, lds);
    if (threadIdx.x == 0) partials[blockIdx.x] = s;
}

// pass 2: one workgroup; thread j adds partials[j], [j + 256], ... in that order.  out = {total, coef}:
// total = (float)(grad_scale * sqrt(sum)), coef = min(1, max_norm / (total + 1e-6f)) with torch.clamp's NaN (it stays).
__global__ __launch_bounds__(256) void grad_norm_finish_kernel(const double* __restrict__ partials, int n,
                                                               float grad_scale, const float* __restrict__ hyper,
                                                               float max_norm, float* __restrict__ out) {
    __shared__ double lds[4];
    double acc = 0.0;
    for (int i = threadIdx.x; i < n; i += 256) acc += partials[i];
    const double s = block_sum_d(acc, lds);
    if (threadIdx.x == 0) {
        const float gs = hyper ? hyper[6] : grad_scale;
        const float total = (float)((double)gs * sqrt(s));
        const float c = max_norm / (total + 1e-6f);
        out[0] = total;
        out[1] = c > 1.f ? 1.f : c;
    }
}

// g *= *coef over every gradient of the table; nothing is written when the coefficient is exactly 1
__global__ __launch_bounds__(256) void grad_scale_dev_kernel(const ru3d_adam_tensor* __restrict__ tensors,
                                                             const int32_t* __restrict__ block_map, int chunk_elems,
                                                             const float* __restrict__ coef) {
    const TableChunk ch = table_chunk(tensors, block_map, chunk_elems);
    if (!ch.t.grad) return;
    const float c = *coef;
    if (c == 1.f) return;
    grad_walk(ch, true, [&](float v) { return v * c; });
}

// --------------------------------------------------------------------------- entry points
#define RU3D_TABLE_OK(tensors, block_map, nblocks, chunk_elems) \
    ((tensors) && (block_map) && (nblocks) > 0 && (chunk_elems) >= 1024 && ((chunk_elems) % 1024) == 0)

// What every table entry point does: device guard, the table check and the entry's own conditions (`ok`) with the entry's
// own error text (`bad`), one workgroup per block-map pair, launch check under the entry's name (`what`).
template <class... Params, class... Args>
static int launch_table(void (*kernel)(const ru3d_adam_tensor*, const int32_t*, int, Params...), const char* what,
                        const char* bad, bool ok, const ru3d_adam_tensor* tensors, const int32_t* block_map,
                        int nblocks, int chunk_elems, void* stream, Args... args) {
    Ru3dDeviceGuard dev_guard(stream);
    RU3D_REQUIRE(RU3D_TABLE_OK(tensors, block_map, nblocks, chunk_elems) && ok, "%s", bad);
    hipLaunchKernelGGL(kernel, dim3((unsigned)nblocks), dim3(256), 0, as_stream(stream), tensors, block_map, chunk_elems,
                       args...);
    return ru3d_check_launch(what);
}

// ru3d_adam_multi and ru3d_adam_multi_clip share a kernel (and so do their _dev forms): no coefficient is a null one
extern "C" int ru3d_adam_multi(const ru3d_adam_tensor* tensors, const int32_t* block_map, int nblocks, int chunk_elems,
                               float lr, float beta1, float beta2, float eps, float bias_corr1, float bias_corr2,
                               float grad_scale, void* stream) {
    return launch_table(adam_multi_kernel, "adam_multi",
                        "adam_multi: bad argument (chunk_elems must be a positive multiple of 1024)", true, tensors,
                        block_map, nblocks, chunk_elems, stream, lr, beta1, beta2, eps, bias_corr1, sqrtf(bias_corr2),
                        grad_scale, (const float*)nullptr);
}

extern "C" int ru3d_adam_multi_clip(const ru3d_adam_tensor* tensors, const int32_t* block_map, int nblocks,
                                    int chunk_elems, float lr, float beta1, float beta2, float eps, float bias_corr1,
                                    float bias_corr2, float grad_scale, const float* coef, void* stream) {
    return launch_table(adam_multi_kernel, "adam_multi_clip",
                        "adam_multi_clip: bad argument (chunk_elems must be a positive multiple of 1024)",
                        bias_corr1 > 0.f && bias_corr2 > 0.f, tensors, block_map, nblocks, chunk_elems, stream, lr, beta1,
                        beta2, eps, bias_corr1, sqrtf(bias_corr2), grad_scale, coef);
}

extern "C" int ru3d_adam_multi_dev(const ru3d_adam_tensor* tensors, const int32_t* block_map, int nblocks,
                                   int chunk_elems, const float* hyper, void* stream) {
    return launch_table(adam_multi_dev_kernel, "adam_multi_dev",
                        "adam_multi_dev: bad argument (chunk_elems must be a positive multiple of 1024)", hyper != nullptr,
                        tensors, block_map, nblocks, chunk_elems, stream, hyper, (const float*)nullptr);
}

extern "C" int ru3d_adam_multi_clip_dev(const ru3d_adam_tensor* tensors, const int32_t* block_map, int nblocks,
                                        int chunk_elems, const float* hyper, const float* coef, void* stream) {
    return launch_table(adam_multi_dev_kernel, "adam_multi_clip_dev",
                        "adam_multi_clip_dev: bad argument (chunk_elems must be a positive multiple of 1024)",
                        hyper != nullptr, tensors, block_map, nblocks, chunk_elems, stream, hyper, coef);
}

extern "C" int ru3d_adam_multi_amp(const ru3d_adam_tensor* tensors, const int32_t* block_map, int nblocks, int chunk_elems,
                                   const float* hyper, const ru3d_amp_state* amp, void* stream) {
    return launch_table(adam_multi_amp_kernel, "adam_multi_amp",
                        "adam_multi_amp: bad argument (chunk_elems must be a positive multiple of 1024)", hyper && amp,
                        tensors, block_map, nblocks, chunk_elems, stream, hyper, amp);
}

extern "C" int ru3d_adamw_multi(const ru3d_adam_tensor* tensors, const int32_t* block_map, int nblocks, int chunk_elems,
                                float lr, float beta1, float beta2, float eps, float weight_decay, float bias_corr1,
                                float bias_corr2, float grad_scale, const float* coef, void* stream) {
    return launch_table(adamw_multi_kernel, "adamw_multi",
                        "adamw_multi: bad argument (chunk_elems must be a positive multiple of 1024)",
                        lr >= 0.f && eps >= 0.f && weight_decay >= 0.f && bias_corr1 > 0.f && bias_corr2 > 0.f, tensors,
                        block_map, nblocks, chunk_elems, stream, lr, beta1, beta2, eps, weight_decay, bias_corr1,
                        bias_corr2, grad_scale, coef);
}

extern "C" int ru3d_adamw_multi_dev(const ru3d_adam_tensor* tensors, const int32_t* block_map, int nblocks,
                                    int chunk_elems, const float* hyper, const float* coef, void* stream) {
    return launch_table(adamw_multi_dev_kernel, "adamw_multi_dev",
                        "adamw_multi_dev: bad argument (chunk_elems must be a positive multiple of 1024)", hyper != nullptr,
                        tensors, block_map, nblocks, chunk_elems, stream, hyper, coef);
}

extern "C" int ru3d_sgd_multi(const ru3d_adam_tensor* tensors, const int32_t* block_map, int nblocks, int chunk_elems,
                              float lr, float momentum, float weight_decay, int nesterov, float grad_scale,
                              const float* coef, void* stream) {
    return launch_table(sgd_multi_kernel, "sgd_multi",
                        "sgd_multi: bad argument (chunk_elems must be a positive multiple of 1024; nesterov needs momentum)",
                        lr >= 0.f && momentum >= 0.f && weight_decay >= 0.f &&
                            (nesterov == 0 || (nesterov == 1 && momentum > 0.f)),
                        tensors, block_map, nblocks, chunk_elems, stream, lr, momentum, weight_decay,
                        nesterov ? 1.f : 0.f, grad_scale, coef);
}

extern "C" int ru3d_sgd_multi_dev(const ru3d_adam_tensor* tensors, const int32_t* block_map, int nblocks,
                                  int chunk_elems, const float* hyper, const float* coef, void* stream) {
    return launch_table(sgd_multi_dev_kernel, "sgd_multi_dev",
                        "sgd_multi_dev: bad argument (chunk_elems must be a positive multiple of 1024)", hyper != nullptr,
                        tensors, block_map, nblocks, chunk_elems, stream, hyper, coef);
}

extern "C" int ru3d_grad_scale_check(const ru3d_adam_tensor* tensors, const int32_t* block_map, int nblocks,
                                     int chunk_elems, float scale, float* found_inf, void* stream) {
    return launch_table(grad_scale_check_kernel, "grad_scale_check",
                        "grad_scale_check: bad argument (chunk_elems must be a positive multiple of 1024)",
                        found_inf != nullptr, tensors, block_map, nblocks, chunk_elems, stream, scale, found_inf);
}

extern "C" int ru3d_grad_sumsq(const ru3d_adam_tensor* tensors, const int32_t* block_map, int nblocks, int chunk_elems,
                               double* partials, void* stream) {
    return launch_table(grad_sumsq_kernel, "grad_sumsq",
                        "grad_sumsq: bad argument (chunk_elems must be a positive multiple of 1024)", partials != nullptr,
                        tensors, block_map, nblocks, chunk_elems, stream, partials);
}

extern "C" int ru3d_grad_scale_dev(const ru3d_adam_tensor* tensors, const int32_t* block_map, int nblocks,
                                   int chunk_elems, const float* coef, void* stream) {
    return launch_table(grad_scale_dev_kernel, "grad_scale_dev",
                        "grad_scale_dev: bad argument (chunk_elems must be a positive multiple of 1024)", coef != nullptr,
                        tensors, block_map, nblocks, chunk_elems, stream, coef);
}

extern "C" int ru3d_grad_norm_finish(const double* partials, int npartials, float grad_scale, const float* hyper,
                                     float max_norm, float* out, void* stream) {
    Ru3dDeviceGuard dev_guard(stream);
    RU3D_REQUIRE(partials && out && npartials > 0 && max_norm >= 0.f, "grad_norm_finish: bad argument");
    hipLaunchKernelGGL(grad_norm_finish_kernel, dim3(1), dim3(256), 0, as_stream(stream), partials, npartials,
                       grad_scale, hyper, max_norm, out);
    return ru3d_check_launch("grad_norm_finish");
}

extern "C" int ru3d_grad_norm(const ru3d_adam_tensor* tensors, const int32_t* block_map, int nblocks, int chunk_elems,
                              double* partials, float grad_scale, float max_norm, float* out, void* stream) {
    RU3D_REQUIRE(RU3D_TABLE_OK(tensors, block_map, nblocks, chunk_elems) && partials && out && max_norm >= 0.f,
                 "grad_norm: bad argument (chunk_elems must be a positive multiple of 1024)");
    const int rc = ru3d_grad_sumsq(tensors, block_map, nblocks, chunk_elems, partials, stream);
    if (rc) return rc;
    return ru3d_grad_norm_finish(partials, nblocks, grad_scale, nullptr, max_norm, out, stream);
}
