// C-ABI entry points for the convolution family + error plumbing.  Validates shapes on the host
// before anything is launched (a faulting kernel can reset the whole GPU node), builds the
// data-movement geometry and dispatches to the MFMA implicit-GEMM kernels (bf16, MFMA-friendly
// channel counts) or to the generic direct kernels (fp32 parity mode, odd channel counts).
#include "common.h"
#include "conv.h"
#include <string>

#ifndef RU3D_STORAGE_F16   // error plumbing and version: defined once, by the bf16 build

static thread_local std::string g_last_error;

int ru3d_fail(int code, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    g_last_error = buf;
    return code;
}

// launch log (tests): while armed, the names ru3d_check_launch receives on this thread, joined by ';'
static thread_local std::string g_launch_log;
static thread_local bool g_launch_log_armed = false;

int ru3d_check_launch(const char* what) {
    if (g_launch_log_armed) {
        if (!g_launch_log.empty()) g_launch_log += ';';
        g_launch_log += what;
    }
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        ru3d_fail((int)e, "%s: %s", what, hipGetErrorString(e));
        return (int)e > 0 ? (int)e : 1;
    }
    return 0;
}

extern "C" int ru3d_version(void) { return RU3D_VERSION; }
extern "C" const char* ru3d_last_error(void) { return g_last_error.c_str(); }
extern "C" void ru3d_launch_log_begin(void) {
    g_launch_log.clear();
    g_launch_log_armed = true;
}
extern "C" const char* ru3d_launch_log_end(void) {
    g_launch_log_armed = false;
    return g_launch_log.c_str();
}
#endif

namespace RU3D_NS {

static bool dtype_ok(int d) { return d == RU3D_F32 || d == RU3D_BF16; }   // fp32 or this build's 16-bit type
static int conv_out(int in, int k, int s) { return (in + 2 * (k / 2) - k) / s + 1; }

// channels (in', out') of the data-movement kernel that consumes a packed weight
static void role_channels(int cout, int cin, int role, int* kin, int* kout, int64_t* s_o, int64_t* s_i, int taps) {
    switch (role) {
        case RU3D_ROLE_CONV_FWD:  // W[co][ci][tap]
            *kin = cin; *kout = cout; *s_o = (int64_t)cin * taps; *s_i = taps; break;
        case RU3D_ROLE_CONV_DGRAD:  // in' = co, out' = ci
            *kin = cout; *kout = cin; *s_o = taps; *s_i = (int64_t)cin * taps; break;
        case RU3D_ROLE_CONVT_FWD:  // W[ci][co][tap], in' = ci, out' = co
            *kin = cin; *kout = cout; *s_o = taps; *s_i = (int64_t)cout * taps; break;
        default:  // CONVT_DGRAD: in' = co, out' = ci
            *kin = cout; *kout = cin; *s_o = (int64_t)cout * taps; *s_i = taps; break;
    }
}

// does the kernel that will consume this packed weight run on the MFMA path?  (all forms; channel counts decide)
static bool role_uses_mfma(int kin, int kout, int k, int stride, int role, int dtype) {
    (void)stride;
    (void)role;
    return mfma_conv_eligible(kin, kout, k, dtype, dtype);
}

extern "C" size_t ru3d_packed_weight_bytes(int cout, int cin, int k, int stride, int role, int dtype) {
    RU3D_FWD_F16(dtype, ru3d_packed_weight_bytes_f16(cout, cin, k, stride, role, dtype));
    if (cout <= 0 || cin <= 0 || (k != 1 && k != 3) || (stride != 1 && stride != 2) || role < 0 || role > 3 ||
        !dtype_ok(dtype))
        return 0;
    const int taps = k * k * k;
    int kin, kout;
    int64_t s_o, s_i;
    role_channels(cout, cin, role, &kin, &kout, &s_o, &s_i, taps);
    if (role_uses_mfma(kin, kout, k, stride, role, dtype)) return mfma_packed_bytes(kin, kout, taps);
    return (size_t)taps * kin * generic_cout_pad(kout) * (dtype == RU3D_F32 ? 4 : 2);
}

extern "C" int ru3d_pack_weight(const float* src, void* dst, int cout, int cin, int k, int stride, int role, int dtype,
                                void* stream) {
    RU3D_FWD_F16(dtype, ru3d_pack_weight_f16(src, dst, cout, cin, k, stride, role, dtype, stream));
    Ru3dDeviceGuard dev_guard(stream);
    RU3D_REQUIRE(src && dst, "pack_weight: null pointer");
    RU3D_REQUIRE(cout > 0 && cin > 0 && (k == 1 || k == 3) && (stride == 1 || stride == 2),
                 "pack_weight: bad shape cout=%d cin=%d k=%d stride=%d", cout, cin, k, stride);
    RU3D_REQUIRE(role >= 0 && role <= 3 && dtype_ok(dtype), "pack_weight: bad role/dtype");
    const int taps = k * k * k;
    int kin, kout;
    int64_t s_o, s_i;
    role_channels(cout, cin, role, &kin, &kout, &s_o, &s_i, taps);
    if (role_uses_mfma(kin, kout, k, stride, role, dtype))
        return pack_mfma_launch(src, dst, kin, kout, taps, s_o, s_i, 0, as_stream(stream));
    return pack_generic_launch(src, dst, kin, kout, taps, s_o, s_i, 0, dtype, as_stream(stream));
}

static int pad32(int c) { return (c + 31) / 32 * 32; }
// packed extent of a module dimension of `real` channels made of segments of `seg` (0: no padding)
static int padded_dim(int real, int seg) { return seg > 0 ? (real / seg) * pad32(seg) : real; }

extern "C" int ru3d_pack_weights(const ru3d_pack_item* items, int count, int dtype, void* stream) {
    RU3D_FWD_F16(dtype, ru3d_pack_weights_f16(items, count, dtype, stream));
    Ru3dDeviceGuard dev_guard(stream);
    RU3D_REQUIRE(items && count > 0 && count <= RU3D_PACK_MAX, "pack_weights: count must be 1..%d", RU3D_PACK_MAX);
    RU3D_REQUIRE(dtype_ok(dtype), "pack_weights: bad dtype");
    PackBatch b;
    b.count = count;
    for (int i = 0; i < count; i++) {
        const ru3d_pack_item& it = items[i];
        RU3D_REQUIRE(it.src && it.dst && it.cout > 0 && it.cin > 0 && (it.k == 1 || it.k == 3) &&
                         (it.stride == 1 || it.stride == 2) && it.role >= 0 && it.role <= RU3D_ROLE_BIAS,
                     "pack_weights: bad item %d", i);
        RU3D_REQUIRE(it.cout_seg >= 0 && it.cin_seg >= 0 && (it.cout_seg == 0 || it.cout % it.cout_seg == 0) &&
                         (it.cin_seg == 0 || it.cin % it.cin_seg == 0),
                     "pack_weights: item %d: segments (%d, %d) do not divide (%d, %d)", i, it.cout_seg, it.cin_seg,
                     it.cout, it.cin);
        PackOne& p = b.item[i];
        p.src = it.src;
        p.dst = it.dst;
        if (it.role == RU3D_ROLE_BIAS) {
            p.mfma = 2;
            p.cout = padded_dim(it.cout, it.cout_seg);
            p.cin = 1; p.taps = 1; p.cout_pad = p.cout; p.s_o = 1; p.s_i = 1;
            p.co_real = it.cout_seg; p.co_pad = it.cout_seg ? pad32(it.cout_seg) : 0;
            p.ci_real = 0; p.ci_pad = 0;
            p.total = p.cout;
            continue;
        }
        const int taps = it.k * it.k * it.k;
        int kin, kout;
        int64_t s_o, s_i;
        role_channels(it.cout, it.cin, it.role, &kin, &kout, &s_o, &s_i, taps);   // strides: of the REAL source
        // which module dimension is the kernel's input / output channel dimension
        const bool in_is_cin = (it.role == RU3D_ROLE_CONV_FWD || it.role == RU3D_ROLE_CONVT_FWD);
        const int kin_seg = in_is_cin ? it.cin_seg : it.cout_seg, kout_seg = in_is_cin ? it.cout_seg : it.cin_seg;
        const int kin_p = padded_dim(kin, kin_seg), kout_p = padded_dim(kout, kout_seg);
        p.cin = kin_p; p.cout = kout_p; p.taps = taps; p.s_o = s_o; p.s_i = s_i;
        p.ci_real = kin_seg; p.ci_pad = kin_seg ? pad32(kin_seg) : 0;
        p.co_real = kout_seg; p.co_pad = kout_seg ? pad32(kout_seg) : 0;
        p.mfma = role_uses_mfma(kin_p, kout_p, it.k, it.stride, it.role, dtype) ? 1 : 0;
        p.cout_pad = generic_cout_pad(kout_p);
        p.total = p.mfma ? (int64_t)taps * kin_p * kout_p : (int64_t)taps * kin_p * p.cout_pad;
    }
    // MFMA forms whose packed extents are multiples of 32 go through the fused kernel: one read of the source serves the
    // forward and the input-gradient role of the same weight (the usual request: a ResBlock packs both for each conv)
    PackPairBatch pairs;
    pairs.count = 0;
    if (dtype == RU3D_BF16) {
        for (int i = 0; i < count; i++) {
            PackOne& p = b.item[i];
            const ru3d_pack_item& it = items[i];
            if (p.mfma != 1 || (p.cin % 32) || (p.cout % 32) || (p.taps != 27 && p.taps != 1)) continue;
            // source [a][b][tap]: Conv3d a = cout, ConvTranspose3d a = cin; a-major form = the role whose kout is a
            const bool is_t = it.role == RU3D_ROLE_CONVT_FWD || it.role == RU3D_ROLE_CONVT_DGRAD;
            const bool a_major = it.role == RU3D_ROLE_CONV_FWD || it.role == RU3D_ROLE_CONVT_DGRAD;
            const int a_seg = is_t ? it.cin_seg : it.cout_seg, b_seg = is_t ? it.cout_seg : it.cin_seg;
            const int a_realdim = is_t ? it.cin : it.cout, b_realdim = is_t ? it.cout : it.cin;
            int slot = -1;
            for (int j = 0; j < pairs.count; j++)
                if (pairs.item[j].src == it.src && pairs.item[j].taps == p.taps &&
                    pairs.item[j].adim == padded_dim(a_realdim, a_seg) && pairs.item[j].bdim == padded_dim(b_realdim, b_seg) &&
                    pairs.item[j].a_real == a_seg && pairs.item[j].b_real == b_seg &&
                    (a_major ? !pairs.item[j].dst_a : !pairs.item[j].dst_b))
                    slot = j;
            if (slot < 0) {
                slot = pairs.count++;
                PackPair& q = pairs.item[slot];
                q.src = it.src; q.dst_a = nullptr; q.dst_b = nullptr;
                q.adim = padded_dim(a_realdim, a_seg); q.bdim = padded_dim(b_realdim, b_seg); q.taps = p.taps;
                q.a_real = a_seg; q.a_pad = a_seg ? pad32(a_seg) : 0;
                q.b_real = b_seg; q.b_pad = b_seg ? pad32(b_seg) : 0;
                q.s_a = (int64_t)b_realdim * p.taps;
            }
            (a_major ? pairs.item[slot].dst_a : pairs.item[slot].dst_b) = p.dst;
            p.mfma = 3;   // handled by the fused kernel: pack_batch_kernel skips it
        }
    }
    bool rest = false;
    for (int i = 0; i < count; i++) rest = rest || b.item[i].mfma != 3;
    if (pairs.count) {
        int rc = pack_pair_launch(pairs, as_stream(stream));
        if (rc || !rest) return rc;
    }
    return pack_batch_launch(b, dtype, as_stream(stream));
}

#ifndef RU3D_STORAGE_F16
extern "C" int ru3d_unpad_weight_grad(const float* src, float* dst, int cout, int cin, int taps, int cout_seg,
                                      int cin_seg, void* stream) {
    Ru3dDeviceGuard dev_guard(stream);
    RU3D_REQUIRE(src && dst && cout > 0 && cin > 0 && taps > 0, "unpad_weight_grad: bad argument");
    RU3D_REQUIRE(cout_seg >= 0 && cin_seg >= 0 && (cout_seg == 0 || cout % cout_seg == 0) &&
                     (cin_seg == 0 || cin % cin_seg == 0), "unpad_weight_grad: bad segments");
    return unpad_weight_launch(src, dst, cout, cin, taps, cout_seg, cout_seg ? pad32(cout_seg) : 0, cin_seg,
                               cin_seg ? pad32(cin_seg) : 0, padded_dim(cin, cin_seg), as_stream(stream));
}
#endif

// the geometry of the data-movement form: x is what the kernel gathers from, y what it writes
static ConvGeom conv_geom(const ru3d_tensor* x, const ru3d_tensor* y, const ru3d_tensor* res, int k, int stride,
                          int transposed = 0, int flip = 0, int zero_far = 0) {
    ConvGeom g;
    g.N = x->n;
    g.Di = x->d; g.Hi = x->h; g.Wi = x->w; g.Cin = x->c; g.ldx = x->ld;
    g.Do = y->d; g.Ho = y->h; g.Wo = y->w; g.Cout = y->c; g.ldy = y->ld;
    g.CoutPad = generic_cout_pad(y->c);
    g.ldr = res ? res->ld : 0;
    g.k = k; g.stride = stride; g.pad = k / 2;
    g.transposed = transposed; g.zero_far = zero_far; g.flip = flip;
    g.x_cseg = x->cseg; g.x_segstride = x->seg_stride; g.y_cseg = y->cseg; g.y_segstride = y->seg_stride;
    return g;
}
static ConvGeom fwd_geom(const ru3d_tensor* x, const ru3d_tensor* y, int k, int stride) { return conv_geom(x, y, nullptr, k, stride); }
// the stride-1 input gradient: gather form with reversed taps
static ConvGeom dgrad_s1_geom(const ru3d_tensor* dy, const ru3d_tensor* da, int k) { return conv_geom(dy, da, nullptr, k, 1, 0, 1); }

// The plan of the 3x3x3 stride-1 MFMA conv of this geometry (conv.h); empty - nothing fused, no scratch - for every other
// form and dtype.  An entry point makes it once and hands it to whatever it asks and launches.
static Conv3S1Plan s1_plan_for(const ConvGeom& g, int dtype) {
    return mfma_conv_eligible(g.Cin, g.Cout, g.k, dtype, dtype) ? conv3_s1_plan(g) : Conv3S1Plan();
}

static int run_conv(const ru3d_tensor* x, const void* w, const float* bias, const ru3d_tensor* res,
                    const ru3d_tensor* y, int k, int stride, int transposed, int flip, int zero_far, int dtype,
                    int y_dtype, hipStream_t st, void* ws = nullptr, size_t ws_bytes = 0) {
    const ConvGeom g = conv_geom(x, y, res, k, stride, transposed, flip, zero_far);
    if (g.x_cseg || g.y_cseg) {      // the planar concat: only the MFMA conv kernels of a decoder ResBlock take it
        if (!(mfma_conv_eligible(g.Cin, g.Cout, k, dtype, y_dtype) && mfma_conv_geometry_ok(g)))
            return ru3d_fail(-1, "conv3d: no kernel takes a split tensor for this shape / dtype");
        return conv_mfma_launch(x->ptr, w, bias, res ? res->ptr : nullptr, y->ptr, g, st, nullptr, ws, ws_bytes);
    }
    if (stem_fwd_eligible(g, dtype, y_dtype, res)) return stem_fwd_launch(x->ptr, w, bias, y->ptr, g, dtype, st);
    if (head_fwd_eligible(g, dtype, res)) return head_fwd_launch(x->ptr, w, bias, y->ptr, g, dtype, y_dtype, st);
    if (!bias && head_dgrad_eligible(g, dtype, y_dtype, res)) return head_dgrad_launch(x->ptr, w, y->ptr, g, dtype, st);
    if (mfma_conv_eligible(g.Cin, g.Cout, k, dtype, y_dtype) && mfma_conv_geometry_ok(g))
        return conv_mfma_launch(x->ptr, w, bias, res ? res->ptr : nullptr, y->ptr, g, st, nullptr, ws, ws_bytes);
    // ru3d_pack_weight(s) chose the MFMA fragment layout from (channels, k, dtype) alone: a conv of such a shape that
    // cannot take the MFMA path (16-bit input with an fp32 output other than the small head) must not hand that pack to
    // the direct kernel, which expects [tap][cin][cout_pad]
    if (mfma_conv_eligible(g.Cin, g.Cout, k, dtype, dtype))
        return ru3d_fail(-1, "conv3d: %d -> %d channels k=%d is packed in MFMA fragment order, which has no kernel for "
                             "input dtype %d -> output dtype %d", g.Cin, g.Cout, k, dtype, y_dtype);
    return conv_generic_launch(x->ptr, w, bias, res ? res->ptr : nullptr, y->ptr, g, dtype, y_dtype, st);
}

static bool res_ok(const ru3d_tensor* res, const ru3d_tensor* y) {
    return !res || (tensor_ok(res) && res->n == y->n && res->d == y->d && res->h == y->h && res->w == y->w &&
                    res->c == y->c);
}

// Optional scratch of a conv launch (split-K partials of the deepest level); 0 for most shapes.  The same figure serves
// the input gradient of a stride-1 conv (call it with (dy, dx)).
extern "C" size_t ru3d_conv3d_workspace_bytes(const ru3d_tensor* x, const ru3d_tensor* y, int k, int stride, int dtype) {
    RU3D_FWD_F16(dtype, ru3d_conv3d_workspace_bytes_f16(x, y, k, stride, dtype));
    if (!tensor_ok_split(x) || !tensor_ok(y) || dtype != RU3D_BF16 || k != 3 || stride != 1) return 0;
    return s1_plan_for(fwd_geom(x, y, k, stride), dtype).ws_bytes;
}

// Which kernels a conv of this geometry runs on, in the order of preference, joined by '|': run_conv's routing for dense
// tensors of one dtype without a residual, then the MFMA family's plan.  Pure host code; no pointer is dereferenced.
extern "C" int ru3d_conv3d_plan_names(const ru3d_tensor* x, const ru3d_tensor* y, int k, int stride, int transposed,
                                      int dtype, char* buf, size_t cap) {
    RU3D_FWD_F16(dtype, ru3d_conv3d_plan_names_f16(x, y, k, stride, transposed, dtype, buf, cap));
    RU3D_REQUIRE(tensor_ok(x) && tensor_ok(y) && x->n == y->n && buf && cap > 0, "conv3d_plan_names: bad argument");
    RU3D_REQUIRE((k == 1 || k == 3) && (stride == 1 || stride == 2) && dtype_ok(dtype) && (!transposed || stride == 2),
                 "conv3d_plan_names: k=%d stride=%d transposed=%d dtype=%d unsupported", k, stride, transposed, dtype);
    const ConvGeom g = conv_geom(x, y, nullptr, k, stride, transposed ? 1 : 0);
    std::string s;
    if (stem_fwd_eligible(g, dtype, dtype, nullptr)) s = "stem";
    else if (head_fwd_eligible(g, dtype, nullptr) || head_dgrad_eligible(g, dtype, dtype, nullptr)) s = "head";
    else if (!mfma_conv_eligible(g.Cin, g.Cout, k, dtype, dtype)) s = "generic";
    else if (const Conv3S1Plan p = conv3_s1_plan(g); p.count) {
        for (int i = 0; i < p.count; i++) s += std::string(i ? "|" : "") + p.choice[i].name;
    } else {
        const ConvDirectPlan d = conv_direct_plan(g);
        RU3D_REQUIRE(d.family, "%s", d.refusal);
        s = d.tile ? std::string(d.tile_name) + "|" + d.name : std::string(d.name);
    }
    snprintf(buf, cap, "%s", s.c_str());
    return 0;
}

extern "C" int ru3d_conv3d_fwd(const ru3d_tensor* x, const void* w_packed, const float* bias, const ru3d_tensor* res,
                               const ru3d_tensor* y, int k, int stride, int dtype, int y_dtype, void* ws,
                               size_t ws_bytes, void* stream) {
    RU3D_FWD_F16(dtype, ru3d_conv3d_fwd_f16(x, w_packed, bias, res, y, k, stride, dtype, y_dtype, ws, ws_bytes, stream));
    Ru3dDeviceGuard dev_guard(stream);
    RU3D_REQUIRE(tensor_ok_split(x) && tensor_ok(y) && w_packed, "conv3d_fwd: bad tensor/weight");
    RU3D_REQUIRE((k == 1 || k == 3) && (stride == 1 || stride == 2), "conv3d_fwd: k=%d stride=%d unsupported", k, stride);
    RU3D_REQUIRE(dtype_ok(dtype) && dtype_ok(y_dtype) && !(dtype == RU3D_F32 && y_dtype == RU3D_BF16),
                 "conv3d_fwd: bad dtypes %d -> %d", dtype, y_dtype);
    RU3D_REQUIRE(x->n == y->n && y->d == conv_out(x->d, k, stride) && y->h == conv_out(x->h, k, stride) &&
                     y->w == conv_out(x->w, k, stride),
                 "conv3d_fwd: output extents (%d,%d,%d) do not match input (%d,%d,%d) k=%d s=%d", y->d, y->h, y->w,
                 x->d, x->h, x->w, k, stride);
    RU3D_REQUIRE(res_ok(res, y), "conv3d_fwd: residual shape mismatch");
    return run_conv(x, w_packed, bias, res, y, k, stride, 0, 0, 0, dtype, y_dtype, as_stream(stream), ws, ws_bytes);
}

// scratch of ru3d_conv3d_fwd_in: the statistics pass's or the fused slab, and the conv's split-K partials (stream order keeps
// them apart)
static size_t fwd_in_ws_bytes(const ru3d_tensor* y, const Conv3S1Plan& p) {
    size_t need = ru3d_reduce_workspace_bytes(y);
    if (p.can_stats && p.slab_bytes > need) need = p.slab_bytes;
    return p.ws_bytes > need ? p.ws_bytes : need;
}

extern "C" size_t ru3d_conv3d_fwd_in_workspace_bytes(const ru3d_tensor* x, const ru3d_tensor* y, int k, int stride,
                                                     int dtype) {
    RU3D_FWD_F16(dtype, ru3d_conv3d_fwd_in_workspace_bytes_f16(x, y, k, stride, dtype));
    if (!tensor_ok_split(x) || !tensor_ok(y)) return 0;
    return fwd_in_ws_bytes(y, s1_plan_for(fwd_geom(x, y, k, stride), dtype));
}

static int conv_fwd_in(const ru3d_tensor* x, const void* w_packed, const float* bias, const ru3d_tensor* y, int k, int stride,
                       int dtype, const float* drop_scale, float* mean, float* scale, void* ws, size_t ws_bytes, float eps,
                       void* stream, const ConvGeom& g, const Conv3S1Plan& p) {
    RU3D_REQUIRE(ws_bytes >= fwd_in_ws_bytes(y, p), "conv3d_fwd_in: workspace too small");
    if (p.can_stats) {
        RU3D_REQUIRE(x->n == y->n && y->d == x->d && y->h == x->h && y->w == x->w, "conv3d_fwd_in: extents mismatch");
        int rc = conv_mfma_launch(x->ptr, w_packed, bias, nullptr, y->ptr, g, as_stream(stream), (float*)ws, nullptr, 0, nullptr,
                                  0, 0.f, nullptr, 0, nullptr, nullptr, &p);
        if (rc) return rc;
        return stats_slab_finalize_launch((const float*)ws, p.gx, p.cb, g.N, g.Cout, 1.0 / ((double)g.Do * g.Ho * g.Wo),
                                          drop_scale, eps, mean, scale, as_stream(stream));
    }
    // the conv's split-K partials and the statistics pass share the workspace (stream order keeps them apart)
    int rc = ru3d_conv3d_fwd(x, w_packed, bias, nullptr, y, k, stride, dtype, dtype, ws, ws_bytes, stream);
    if (rc) return rc;
    return ru3d_instnorm_stats(y, drop_scale, mean, scale, ws, ws_bytes, eps, dtype, stream);
}

extern "C" int ru3d_conv3d_fwd_in(const ru3d_tensor* x, const void* w_packed, const float* bias, const ru3d_tensor* y,
                                  int k, int stride, int dtype, const float* drop_scale, float* mean, float* scale,
                                  void* ws, size_t ws_bytes, float eps, void* stream) {
    RU3D_FWD_F16(dtype, ru3d_conv3d_fwd_in_f16(x, w_packed, bias, y, k, stride, dtype, drop_scale, mean, scale, ws, ws_bytes, eps, stream));
    Ru3dDeviceGuard dev_guard(stream);
    RU3D_REQUIRE(tensor_ok_split(x) && tensor_ok(y) && w_packed && mean && scale && ws, "conv3d_fwd_in: bad argument");
    const ConvGeom g = fwd_geom(x, y, k, stride);
    return conv_fwd_in(x, w_packed, bias, y, k, stride, dtype, drop_scale, mean, scale, ws, ws_bytes, eps, stream, g,
                       s1_plan_for(g, dtype));
}

// ---- conv + InstanceNorm statistics + apply (+ residual) + LeakyReLU behind one entry point (reference network.py:
// 405-416: x = lrelu(IN(dropout(conv1(x)))), lrelu(IN(conv2(x)) + skip)).  On the small levels the statistics, their
// finalize and the apply are ONE whole-instance kernel (norm_small.hip) that also sums the conv's split-K slices;
// everywhere else this is ru3d_conv3d_fwd_in followed by ru3d_in_lrelu_fwd.
static bool small_conv_path(const ConvGeom& g, const Conv3S1Plan& p, int dtype) {
    return g.k == 3 && g.stride == 1 && mfma_conv_eligible(g.Cin, g.Cout, g.k, dtype, dtype) && !p.can_stats;
}

#ifndef RU3D_STORAGE_F16
extern "C" size_t ru3d_conv3d_fwd_in_lrelu_workspace_bytes(const ru3d_tensor* x, const ru3d_tensor* y, int k, int stride,
                                                           int dtype) {
    return ru3d_conv3d_fwd_in_workspace_bytes(x, y, k, stride, dtype);
}
#endif

extern "C" int ru3d_conv3d_fwd_in_lrelu(const ru3d_tensor* x, const void* w_packed, const float* bias, const ru3d_tensor* y,
                                        int k, int stride, int dtype, const float* drop_scale, float* mean, float* scale,
                                        const ru3d_tensor* res, const ru3d_tensor* out, float slope, void* ws,
                                        size_t ws_bytes, float eps, void* stream) {
    RU3D_FWD_F16(dtype, ru3d_conv3d_fwd_in_lrelu_f16(x, w_packed, bias, y, k, stride, dtype, drop_scale, mean, scale, res, out, slope, ws, ws_bytes, eps, stream));
    Ru3dDeviceGuard dev_guard(stream);
    RU3D_REQUIRE(tensor_ok_split(x) && tensor_ok(y) && tensor_ok(out) && w_packed && mean && scale && ws,
                 "conv3d_fwd_in_lrelu: bad argument");
    RU3D_REQUIRE(res_ok(res, y) && res_ok(out, y), "conv3d_fwd_in_lrelu: res / out do not have the shape of y");
    const ConvGeom g = fwd_geom(x, y, k, stride);
    const Conv3S1Plan p = s1_plan_for(g, dtype);
    const int small = (small_conv_path(g, p, dtype) && x->n == y->n && y->d == x->d && y->h == x->h &&
                       y->w == x->w) ? in_small_mode(y, false, res, out) : 0;
    if (small) {
        RU3D_REQUIRE(ws_bytes >= fwd_in_ws_bytes(y, p), "conv3d_fwd_in_lrelu: workspace too small");
        int ks = 0;      // the whole-instance kernel sums the conv's split-K slices itself; the two-kernel form reads y
        int rc = conv_mfma_launch(x->ptr, w_packed, bias, nullptr, y->ptr, g, as_stream(stream), nullptr, ws, ws_bytes, nullptr,
                                  0, 0.f, nullptr, 0, nullptr, small == 1 ? &ks : nullptr, &p);
        if (rc) return rc;
        return in_small_fwd_launch(y, ks ? (const float*)ws : nullptr, ks, bias, drop_scale, mean, scale, res, out, ws, eps,
                                   slope, as_stream(stream));
    }
    int rc = conv_fwd_in(x, w_packed, bias, y, k, stride, dtype, drop_scale, mean, scale, ws, ws_bytes, eps, stream, g, p);
    if (rc) return rc;
    return ru3d_in_lrelu_fwd(y, mean, scale, res, out, slope, dtype, stream);
}

static WgradGeom make_wgrad(const ru3d_tensor* x, const ru3d_tensor* dy, int k, int stride) {
    WgradGeom g;
    g.N = x->n;
    g.Di = x->d; g.Hi = x->h; g.Wi = x->w; g.Cin = x->c; g.ldx = x->ld;
    g.Do = dy->d; g.Ho = dy->h; g.Wo = dy->w; g.Cout = dy->c; g.lddy = dy->ld;
    g.k = k; g.taps = k * k * k; g.stride = stride; g.pad = k / 2;
    g.s_o = (int64_t)x->c * g.taps;
    g.s_i = g.taps;
    g.chunk_len = 0;
    g.x_cseg = x->cseg; g.x_segstride = x->seg_stride;
    return g;
}

// ---- can a decoder ResBlock take cat((up, skip)) as a split tensor through all of its kernels? (see ru3d_tensor)
extern "C" int ru3d_planar_concat_supported(int n, int d, int h, int w, int cseg, int cout, int dtype) {
    RU3D_FWD_F16(dtype, ru3d_planar_concat_supported_f16(n, d, h, w, cseg, cout, dtype));
    static const int mode = ru3d_env_int("RU3D_PLANAR_CONCAT", 1), pair_mode = ru3d_env_int("RU3D_DGRAD_PAIR", 1);
    static const int skip_mode = ru3d_env_int("RU3D_FUSED_SKIP", 1);
    if (!mode || dtype != RU3D_BF16 || n <= 0 || d <= 0 || h <= 0 || w <= 0 || cseg != 32 || cout != 32) return 0;
    const int64_t V = (int64_t)d * h * w;
    // byte offsets of the sliding kernel's staging: plane distance + one sample below 2^31
    if (((int64_t)n * V + V) * cseg * 2 >= (1ll << 31)) return 0;
    const ru3d_tensor cat = {nullptr, n, d, h, w, 2 * cseg, cseg, 0, 0}, act = {nullptr, n, d, h, w, cout, cout, 0, 0};
    const Conv3S1Plan fwd = conv3_s1_plan(fwd_geom(&cat, &act, 3, 1));                 // conv1 forward (split input)
    if (!fwd.count || fwd.choice[0].family != S1_SLIDE64) return 0;
    const ConvGeom gd = dgrad_s1_geom(&act, &cat, 3);                                  // its input-gradient pair (split output)
    if (!pair_mode || !s1_plan_for(gd, dtype).can_partner) return 0;
    if (wgrad_plan(make_wgrad(&cat, &act, 3, 1), dtype).family != WG_SLIDE) return 0;   // conv1's weight gradient (split x)
    // the fused tail (skip conv + InstanceNorm apply): skip1x1_fused_eligible's shape conditions
    if (!skip_mode || (V % 16) != 0 || V * n < 65536) return 0;
    return 1;
}

extern "C" int ru3d_conv3d_dgrad(const ru3d_tensor* dy, const void* w_packed, const ru3d_tensor* res,
                                 const ru3d_tensor* dx, int k, int stride, int dtype, void* ws, size_t ws_bytes,
                                 void* stream) {
    RU3D_FWD_F16(dtype, ru3d_conv3d_dgrad_f16(dy, w_packed, res, dx, k, stride, dtype, ws, ws_bytes, stream));
    Ru3dDeviceGuard dev_guard(stream);
    RU3D_REQUIRE(tensor_ok(dy) && tensor_ok(dx) && w_packed, "conv3d_dgrad: bad tensor/weight");
    RU3D_REQUIRE((k == 1 || k == 3) && (stride == 1 || stride == 2), "conv3d_dgrad: k=%d stride=%d unsupported", k, stride);
    RU3D_REQUIRE(dtype_ok(dtype), "conv3d_dgrad: bad dtype");
    RU3D_REQUIRE(dx->n == dy->n && dy->d == conv_out(dx->d, k, stride) && dy->h == conv_out(dx->h, k, stride) &&
                     dy->w == conv_out(dx->w, k, stride),
                 "conv3d_dgrad: dy extents (%d,%d,%d) do not match dx (%d,%d,%d) k=%d s=%d", dy->d, dy->h, dy->w,
                 dx->d, dx->h, dx->w, k, stride);
    RU3D_REQUIRE(res_ok(res, dx), "conv3d_dgrad: residual shape mismatch");
    // stride 1: gather form with reversed taps; stride 2: transposed (fractionally strided) form
    if (stride == 1)
        return run_conv(dy, w_packed, nullptr, res, dx, k, 1, 0, 1, 0, dtype, dtype, as_stream(stream), ws, ws_bytes);
    return run_conv(dy, w_packed, nullptr, res, dx, k, stride, 1, 0, 0, dtype, dtype, as_stream(stream));
}

// ---- decoder ResBlock: input gradient of conv1 (k3 s1) and skip_conv (k1 s1) in one launch (conv_slide32.hip, 28th tap)
extern "C" int ru3d_conv3d_s1_dgrad_pair_supported(const ru3d_tensor* dy, const ru3d_tensor* dy2, const ru3d_tensor* dx, int dtype) {
    RU3D_FWD_F16(dtype, ru3d_conv3d_s1_dgrad_pair_supported_f16(dy, dy2, dx, dtype));
    static const int mode = ru3d_env_int("RU3D_DGRAD_PAIR", 1);
    if (!mode || dtype != RU3D_BF16 || !tensor_ok(dy) || !tensor_ok(dy2) || !tensor_ok_split(dx)) return 0;
    if (dx->cseg && (dx->cseg != 32 || dx->c != 64)) return 0;      // split output: two 32-channel slices, one per grid row
    if (dy2->n != dy->n || dy2->d != dy->d || dy2->h != dy->h || dy2->w != dy->w || dy2->c != dy->c) return 0;
    if (dx->n != dy->n || dx->d != dy->d || dx->h != dy->h || dx->w != dy->w) return 0;
    if ((dy->ld % 8) || (dy2->ld % 8) || (dx->ld % 8)) return 0;
    if ((((uintptr_t)dy->ptr) | ((uintptr_t)dy2->ptr) | ((uintptr_t)dx->ptr)) % 16) return 0;
    if ((int64_t)dy->d * dy->h * dy->w * dy->ld >= (1ll << 30)) return 0;
    return s1_plan_for(dgrad_s1_geom(dy, dx, 3), dtype).can_partner ? 1 : 0;
}

extern "C" int ru3d_conv3d_s1_dgrad_pair(const ru3d_tensor* dy, const void* w3_packed, const ru3d_tensor* dy2,
                                         const void* w1_packed, const ru3d_tensor* dx, int dtype, void* stream) {
    RU3D_FWD_F16(dtype, ru3d_conv3d_s1_dgrad_pair_f16(dy, w3_packed, dy2, w1_packed, dx, dtype, stream));
    Ru3dDeviceGuard dev_guard(stream);
    RU3D_REQUIRE(w3_packed && w1_packed, "conv3d_s1_dgrad_pair: null weight");
    RU3D_REQUIRE(ru3d_conv3d_s1_dgrad_pair_supported(dy, dy2, dx, dtype),
                 "conv3d_s1_dgrad_pair: shapes have no fused kernel (ask ru3d_conv3d_s1_dgrad_pair_supported first)");
    const ConvGeom g = dgrad_s1_geom(dy, dx, 3);
    return conv_mfma_launch(dy->ptr, w3_packed, nullptr, nullptr, dx->ptr, g, as_stream(stream), nullptr, nullptr, 0, nullptr, 0,
                            0.f, dy2->ptr, dy2->ld, w1_packed);
}

// ---- decoder ResBlock tail: skip conv + InstanceNorm apply + sum + LeakyReLU (fused_skip.hip)
extern "C" int ru3d_skip1x1_in_lrelu_fwd_supported(const ru3d_tensor* x, const ru3d_tensor* y, const ru3d_tensor* out, int dtype) {
    RU3D_FWD_F16(dtype, ru3d_skip1x1_in_lrelu_fwd_supported_f16(x, y, out, dtype));
    return skip1x1_fused_eligible(x, y, out, dtype) ? 1 : 0;
}

extern "C" int ru3d_skip1x1_in_lrelu_fwd(const ru3d_tensor* x, const void* w_packed, const float* bias, const ru3d_tensor* y,
                                         const float* mean, const float* scale, const ru3d_tensor* out, float slope, int dtype,
                                         void* stream) {
    RU3D_FWD_F16(dtype, ru3d_skip1x1_in_lrelu_fwd_f16(x, w_packed, bias, y, mean, scale, out, slope, dtype, stream));
    Ru3dDeviceGuard dev_guard(stream);
    RU3D_REQUIRE(w_packed && mean && scale, "skip1x1_in_lrelu_fwd: null argument");
    RU3D_REQUIRE(skip1x1_fused_eligible(x, y, out, dtype),
                 "skip1x1_in_lrelu_fwd: shapes have no fused kernel (ask ru3d_skip1x1_in_lrelu_fwd_supported first)");
    return skip1x1_fused_launch(x, w_packed, bias, y, mean, scale, out, slope, as_stream(stream));
}

// the same pass with the network's head on its output: the logits leave the kernel's epilogue
extern "C" int ru3d_skip1x1_in_lrelu_head_fwd_supported(const ru3d_tensor* x, const ru3d_tensor* y, const ru3d_tensor* out,
                                                        const ru3d_tensor* logits, int dtype) {
    RU3D_FWD_F16(dtype, ru3d_skip1x1_in_lrelu_head_fwd_supported_f16(x, y, out, logits, dtype));
    return skip1x1_head_fused_eligible(x, y, out, logits, dtype) ? 1 : 0;
}

extern "C" int ru3d_skip1x1_in_lrelu_head_fwd(const ru3d_tensor* x, const void* w_packed, const float* bias,
                                              const ru3d_tensor* y, const float* mean, const float* scale,
                                              const ru3d_tensor* out, const void* head_w_packed, const float* head_bias,
                                              const ru3d_tensor* logits, float slope, int dtype, void* stream) {
    RU3D_FWD_F16(dtype, ru3d_skip1x1_in_lrelu_head_fwd_f16(x, w_packed, bias, y, mean, scale, out, head_w_packed, head_bias,
                                                           logits, slope, dtype, stream));
    Ru3dDeviceGuard dev_guard(stream);
    RU3D_REQUIRE(w_packed && mean && scale && head_w_packed, "skip1x1_in_lrelu_head_fwd: null argument");
    RU3D_REQUIRE(skip1x1_head_fused_eligible(x, y, out, logits, dtype),
                 "skip1x1_in_lrelu_head_fwd: shapes have no fused kernel (ask ru3d_skip1x1_in_lrelu_head_fwd_supported first)");
    RU3D_REQUIRE((((uintptr_t)head_w_packed) % 8) == 0, "skip1x1_in_lrelu_head_fwd: the head's pack must be 8-byte aligned");
    return skip1x1_fused_launch(x, w_packed, bias, y, mean, scale, out, slope, as_stream(stream), head_w_packed, head_bias,
                                logits);
}

// ---- the two stride-2 convs of a pooling ResBlock: forward of both + InstanceNorm sums in one launch (conv_s2.hip, G form)
// the conditions on the three tensors, then the plan's tile kernel and its launch-time conditions; *g / *p: for the caller
static bool s2_pair_fwd_ok(const ru3d_tensor* x, const ru3d_tensor* y3, const ru3d_tensor* y1, int dtype, ConvGeom* g,
                           ConvDirectPlan* p) {
    if (dtype != RU3D_BF16 || !tensor_ok(x) || !tensor_ok(y3) || !tensor_ok(y1)) return false;
    if (y3->n != x->n || y3->d != conv_out(x->d, 3, 2) || y3->h != conv_out(x->h, 3, 2) || y3->w != conv_out(x->w, 3, 2)) return false;
    if (y1->n != y3->n || y1->d != y3->d || y1->h != y3->h || y1->w != y3->w || y1->c != y3->c) return false;
    *g = fwd_geom(x, y3, 3, 2);
    *p = conv_direct_plan(*g);
    return p->tile == S2_TILE_G && conv_direct_tile_ok(*p, *g, x->ptr, nullptr, y3->ptr, y1->ptr, y1->ld);
}

extern "C" int ru3d_conv3d_s2_pair_fwd_in_supported(const ru3d_tensor* x, const ru3d_tensor* y3, const ru3d_tensor* y1, int dtype) {
    RU3D_FWD_F16(dtype, ru3d_conv3d_s2_pair_fwd_in_supported_f16(x, y3, y1, dtype));
    ConvGeom g; ConvDirectPlan p;
    return s2_pair_fwd_ok(x, y3, y1, dtype, &g, &p) ? 1 : 0;
}

extern "C" size_t ru3d_conv3d_s2_pair_fwd_in_workspace_bytes(const ru3d_tensor* x, const ru3d_tensor* y3, int dtype) {
    RU3D_FWD_F16(dtype, ru3d_conv3d_s2_pair_fwd_in_workspace_bytes_f16(x, y3, dtype));
    if (!tensor_ok(x) || !tensor_ok(y3)) return 0;
    return conv_direct_plan(fwd_geom(x, y3, 3, 2)).slab_bytes;
}

extern "C" int ru3d_conv3d_s2_pair_fwd_in(const ru3d_tensor* x, const void* w3_packed, const float* b3, const ru3d_tensor* y3,
                                          const void* w1_packed, const float* b1, const ru3d_tensor* y1,
                                          const float* drop_scale, float* mean, float* scale, void* ws, size_t ws_bytes,
                                          float eps, int dtype, void* stream) {
    RU3D_FWD_F16(dtype, ru3d_conv3d_s2_pair_fwd_in_f16(x, w3_packed, b3, y3, w1_packed, b1, y1, drop_scale, mean, scale, ws, ws_bytes, eps, dtype, stream));
    Ru3dDeviceGuard dev_guard(stream);
    RU3D_REQUIRE(w3_packed && w1_packed && mean && scale && ws, "conv3d_s2_pair_fwd_in: null argument");
    ConvGeom g; ConvDirectPlan p;
    RU3D_REQUIRE(s2_pair_fwd_ok(x, y3, y1, dtype, &g, &p),
                 "conv3d_s2_pair_fwd_in: shapes have no fused kernel (ask ru3d_conv3d_s2_pair_fwd_in_supported first)");
    RU3D_REQUIRE(ws_bytes >= p.slab_bytes, "conv3d_s2_pair_fwd_in: workspace too small");
    int rc = conv_s2_tile_launch(p, x->ptr, w3_packed, b3, y3->ptr, g, (float*)ws, w1_packed, b1, y1->ptr, y1->ld, as_stream(stream));
    if (rc) return rc;
    return stats_slab_finalize_launch((const float*)ws, p.gx, p.cb, g.N, g.Cout, 1.0 / ((double)g.Do * g.Ho * g.Wo), drop_scale, eps,
                                      mean, scale, as_stream(stream));
}

// ---- the two stride-2 convs of a pooling ResBlock: their input gradients in one launch (conv_s2.hip, T form)
static ConvGeom s2_dgrad_geom(const ru3d_tensor* dy, const ru3d_tensor* res, const ru3d_tensor* dx) {
    return conv_geom(dy, dx, res, 3, 2, 1);
}

static bool s2_dgrad_pair_ok(const ru3d_tensor* dy, const ru3d_tensor* dy2, const ru3d_tensor* res, const ru3d_tensor* dx,
                             int dtype, ConvGeom* g, ConvDirectPlan* p) {
    if (dtype != RU3D_BF16 || !tensor_ok(dy) || !tensor_ok(dy2) || !tensor_ok(dx) || !res_ok(res, dx)) return false;
    if (dy2->n != dy->n || dy2->d != dy->d || dy2->h != dy->h || dy2->w != dy->w || dy2->c != dy->c) return false;
    if (dx->n != dy->n || dy->d != conv_out(dx->d, 3, 2) || dy->h != conv_out(dx->h, 3, 2) || dy->w != conv_out(dx->w, 3, 2))
        return false;
    *g = s2_dgrad_geom(dy, res, dx);
    *p = conv_direct_plan(*g);
    return p->tile == S2_TILE_T && conv_direct_tile_ok(*p, *g, dy->ptr, res ? res->ptr : nullptr, dx->ptr, dy2->ptr, dy2->ld);
}

extern "C" int ru3d_conv3d_s2_dgrad_pair_supported(const ru3d_tensor* dy, const ru3d_tensor* dy2, const ru3d_tensor* res,
                                                   const ru3d_tensor* dx, int dtype) {
    RU3D_FWD_F16(dtype, ru3d_conv3d_s2_dgrad_pair_supported_f16(dy, dy2, res, dx, dtype));
    ConvGeom g; ConvDirectPlan p;
    return s2_dgrad_pair_ok(dy, dy2, res, dx, dtype, &g, &p) ? 1 : 0;
}

extern "C" int ru3d_conv3d_s2_dgrad_pair(const ru3d_tensor* dy, const void* w3_packed, const ru3d_tensor* dy2,
                                         const void* w1_packed, const ru3d_tensor* res, const ru3d_tensor* dx, int dtype,
                                         void* stream) {
    RU3D_FWD_F16(dtype, ru3d_conv3d_s2_dgrad_pair_f16(dy, w3_packed, dy2, w1_packed, res, dx, dtype, stream));
    Ru3dDeviceGuard dev_guard(stream);
    RU3D_REQUIRE(w3_packed && w1_packed, "conv3d_s2_dgrad_pair: null weight");
    ConvGeom g; ConvDirectPlan p;
    RU3D_REQUIRE(s2_dgrad_pair_ok(dy, dy2, res, dx, dtype, &g, &p),
                 "conv3d_s2_dgrad_pair: shapes have no fused kernel (ask ru3d_conv3d_s2_dgrad_pair_supported first)");
    return convt_s2_tile_launch(p, dy->ptr, w3_packed, nullptr, res ? res->ptr : nullptr, dx->ptr, g, nullptr, dy2->ptr,
                                dy2->ld, w1_packed, as_stream(stream));
}

// ---- conv input gradient followed by the InstanceNorm + LeakyReLU backward of the tensor it differentiates
static bool dgrad_in_bwd_fused(const ru3d_tensor* dy, const ru3d_tensor* da, const Conv3S1Plan& p, int dtype) {
    static const int mode = ru3d_env_int("RU3D_DGRAD_IN_FUSE", 1);
    return mode && dtype != RU3D_F32 && p.can_bwd_sums && (da->ld % 8) == 0 && (dy->ld % 8) == 0;
}

static size_t dgrad_in_bwd_ws_bytes(const ru3d_tensor* dy, const ru3d_tensor* da, const Conv3S1Plan& p, int dtype) {
    size_t need = ru3d_reduce_workspace_bytes(da);
    if (dgrad_in_bwd_fused(dy, da, p, dtype)) {
        // slab of per-(workgroup, wave) sums, then m12[n][c][2]
        const size_t fused = (p.slab_bytes + 255) / 256 * 256 + (size_t)da->n * da->c * 2 * sizeof(float);
        if (fused > need) need = fused;
    }
    return p.ws_bytes > need ? p.ws_bytes : need;
}

extern "C" size_t ru3d_conv3d_dgrad_in_bwd_workspace_bytes(const ru3d_tensor* dy, const ru3d_tensor* da, int k,
                                                           int stride, int dtype) {
    RU3D_FWD_F16(dtype, ru3d_conv3d_dgrad_in_bwd_workspace_bytes_f16(dy, da, k, stride, dtype));
    if (!tensor_ok(dy) || !tensor_ok(da)) return 0;
    // (a plan only for stride 1: the stride-2 input gradient is the transposed form)
    return dgrad_in_bwd_ws_bytes(dy, da, stride == 1 ? s1_plan_for(dgrad_s1_geom(dy, da, k), dtype) : Conv3S1Plan(), dtype);
}

extern "C" int ru3d_conv3d_dgrad_in_bwd(const ru3d_tensor* dy, const void* w_packed, const ru3d_tensor* act,
                                        const float* mean, const float* scale, const ru3d_tensor* da,
                                        const ru3d_tensor* dyn, int k, int stride, float slope, int dtype, void* ws,
                                        size_t ws_bytes, void* stream) {
    RU3D_FWD_F16(dtype, ru3d_conv3d_dgrad_in_bwd_f16(dy, w_packed, act, mean, scale, da, dyn, k, stride, slope, dtype, ws, ws_bytes, stream));
    Ru3dDeviceGuard dev_guard(stream);
    RU3D_REQUIRE(tensor_ok(dy) && tensor_ok(act) && tensor_ok(da) && tensor_ok(dyn) && w_packed && mean && scale && ws,
                 "conv3d_dgrad_in_bwd: bad argument");
    RU3D_REQUIRE(res_ok(act, da) && res_ok(dyn, da), "conv3d_dgrad_in_bwd: act / dyn do not have the shape of da");
    const ConvGeom g = dgrad_s1_geom(dy, da, k);
    const Conv3S1Plan p = stride == 1 ? s1_plan_for(g, dtype) : Conv3S1Plan();
    RU3D_REQUIRE(ws_bytes >= dgrad_in_bwd_ws_bytes(dy, da, p, dtype), "conv3d_dgrad_in_bwd: workspace too small");
    if (dgrad_in_bwd_fused(dy, da, p, dtype) && (act->ld % 8) == 0 && (((uintptr_t)act->ptr) % 16) == 0 &&
        (((uintptr_t)da->ptr) % 16) == 0 && (((uintptr_t)dy->ptr) % 16) == 0) {
        RU3D_REQUIRE(da->n == dy->n && da->d == dy->d && da->h == dy->h && da->w == dy->w, "conv3d_dgrad_in_bwd: extents mismatch");
        float* m12 = (float*)((char*)ws + (p.slab_bytes + 255) / 256 * 256);
        int rc = conv_mfma_launch(dy->ptr, w_packed, nullptr, nullptr, da->ptr, g, as_stream(stream), (float*)ws, nullptr, 0,
                                  act->ptr, act->ld, slope, nullptr, 0, nullptr, nullptr, &p);
        if (rc) return rc;
        rc = stats_slab_finalize_launch((const float*)ws, p.gx, p.cb, g.N, g.Cout, 1.0 / ((double)g.Do * g.Ho * g.Wo), nullptr,
                                        0.f, m12, nullptr, as_stream(stream));
        if (rc) return rc;
        return ru3d_in_lrelu_bwd_apply(da, act, mean, scale, m12, dyn, slope, 0, dtype, stream);
    }
    // the small levels: the whole InstanceNorm backward is one kernel, which also sums the conv's split-K slices (da is
    // then never stored: nobody else reads it)
    const int small = (stride == 1 && small_conv_path(g, p, dtype) && da->n == dy->n && da->d == dy->d && da->h == dy->h &&
                       da->w == dy->w) ? in_small_mode(act, false, da, dyn) : 0;
    if (small) {
        int ks = 0;
        int rc = conv_mfma_launch(dy->ptr, w_packed, nullptr, nullptr, da->ptr, g, as_stream(stream), nullptr, ws, ws_bytes,
                                  nullptr, 0, 0.f, nullptr, 0, nullptr, small == 1 ? &ks : nullptr, &p);
        if (rc) return rc;
        return in_small_bwd_launch(da, ks ? (const float*)ws : nullptr, ks, act, act, mean, scale, dyn, nullptr, ws, slope, 0,
                                   nullptr, as_stream(stream));
    }
    // not a shape the sliding kernel takes: the two entry points one after the other (they share the workspace in stream order)
    int rc = ru3d_conv3d_dgrad(dy, w_packed, nullptr, da, k, stride, dtype, ws, ws_bytes, stream);
    if (rc) return rc;
    return ru3d_in_lrelu_bwd(da, act, act, mean, scale, dyn, nullptr, ws, ws_bytes, slope, 0, nullptr, nullptr, dtype, stream);
}

static bool wgrad_shapes_ok(const ru3d_tensor* x, const ru3d_tensor* dy, int k, int stride) {
    return tensor_ok_split(x) && tensor_ok(dy) && x->n == dy->n && dy->d == conv_out(x->d, k, stride) &&
           dy->h == conv_out(x->h, k, stride) && dy->w == conv_out(x->w, k, stride);
}

extern "C" size_t ru3d_conv3d_wgrad_workspace_bytes(const ru3d_tensor* x, const ru3d_tensor* dy, int k, int stride,
                                                    int dtype) {
    RU3D_FWD_F16(dtype, ru3d_conv3d_wgrad_workspace_bytes_f16(x, dy, k, stride, dtype));
    if (!wgrad_shapes_ok(x, dy, k, stride)) return 0;
    return wgrad_plan(make_wgrad(x, dy, k, stride), dtype).ws_bytes;
}

extern "C" int ru3d_conv3d_wgrad(const ru3d_tensor* x, const ru3d_tensor* dy, float* dw, void* ws, size_t ws_bytes,
                                 int k, int stride, int dtype, void* stream) {
    RU3D_FWD_F16(dtype, ru3d_conv3d_wgrad_f16(x, dy, dw, ws, ws_bytes, k, stride, dtype, stream));
    Ru3dDeviceGuard dev_guard(stream);
    RU3D_REQUIRE((k == 1 || k == 3) && (stride == 1 || stride == 2), "conv3d_wgrad: k=%d stride=%d unsupported", k, stride);
    RU3D_REQUIRE(wgrad_shapes_ok(x, dy, k, stride), "conv3d_wgrad: x/dy shape mismatch");
    RU3D_REQUIRE(dw && dtype_ok(dtype), "conv3d_wgrad: bad argument");
    const WgradGeom g = make_wgrad(x, dy, k, stride);
    return wgrad_launch(wgrad_plan(g, dtype), x->ptr, dy->ptr, dw, ws, ws_bytes, g, dtype, as_stream(stream));
}

// ---- a ResBlock's two weight gradients on its input x (conv1: 3x3x3, skip_conv: 1x1x1, both with the block's stride;
// network.py:403-409) from ONE pass over x: the sliding (stride 1: wgrad_slide.hip) and the LDS-DMA (stride 2: wgrad_s2.hip)
// weight-gradient kernels have one tap slot of their four waves' 28 free, and the centre tap's rows are the rows the 1x1x1
// conv reads
// the conditions on the three tensors, then the plan's can_pair; *g / *p: the geometry and its plan for the caller
static bool wgrad_pair_ok(const ru3d_tensor* x, const ru3d_tensor* dy, const ru3d_tensor* dy2, int stride, int dtype,
                          WgradGeom* g, WgradPlan* p) {
    static const int mode = ru3d_env_int("RU3D_WGRAD_PAIR", 1);      // 0 = two launches
    if (!x || !dy || !dy2 || !mode || dtype != RU3D_BF16 || (stride != 1 && stride != 2)) return false;
    if (!wgrad_shapes_ok(x, dy, 3, stride) || !tensor_ok(dy2)) return false;
    if (dy2->n != dy->n || dy2->d != dy->d || dy2->h != dy->h || dy2->w != dy->w || dy2->c != dy->c) return false;
    if ((dy2->ld % 8) || ((((uintptr_t)x->ptr) | ((uintptr_t)dy->ptr) | ((uintptr_t)dy2->ptr)) % 16)) return false;
    if ((int64_t)dy->d * dy->h * dy->w * dy2->ld >= (1ll << 30)) return false;
    *g = make_wgrad(x, dy, 3, stride);
    *p = wgrad_plan(*g, dtype);
    return p->can_pair;
}

extern "C" int ru3d_conv3d_wgrad_pair_supported(const ru3d_tensor* x, const ru3d_tensor* dy, const ru3d_tensor* dy2, int stride,
                                                int dtype) {
    RU3D_FWD_F16(dtype, ru3d_conv3d_wgrad_pair_supported_f16(x, dy, dy2, stride, dtype));
    WgradGeom g;
    WgradPlan p;
    return wgrad_pair_ok(x, dy, dy2, stride, dtype, &g, &p) ? 1 : 0;
}

extern "C" size_t ru3d_conv3d_wgrad_pair_workspace_bytes(const ru3d_tensor* x, const ru3d_tensor* dy, const ru3d_tensor* dy2,
                                                         int stride, int dtype) {
    RU3D_FWD_F16(dtype, ru3d_conv3d_wgrad_pair_workspace_bytes_f16(x, dy, dy2, stride, dtype));
    WgradGeom g;
    WgradPlan p;
    return wgrad_pair_ok(x, dy, dy2, stride, dtype, &g, &p) ? p.pair_ws_bytes : 0;
}

extern "C" int ru3d_conv3d_wgrad_pair(const ru3d_tensor* x, const ru3d_tensor* dy, const ru3d_tensor* dy2, float* dw,
                                      float* dw2, void* ws, size_t ws_bytes, int stride, int dtype, void* stream) {
    RU3D_FWD_F16(dtype, ru3d_conv3d_wgrad_pair_f16(x, dy, dy2, dw, dw2, ws, ws_bytes, stride, dtype, stream));
    Ru3dDeviceGuard dev_guard(stream);
    WgradGeom g;
    WgradPlan p;
    RU3D_REQUIRE(wgrad_pair_ok(x, dy, dy2, stride, dtype, &g, &p),
                 "conv3d_wgrad_pair: shapes have no fused kernel (ask ru3d_conv3d_wgrad_pair_supported first)");
    RU3D_REQUIRE(dw && dw2 && ws, "conv3d_wgrad_pair: null output / workspace");
    return wgrad_launch(p, x->ptr, dy->ptr, dw, ws, ws_bytes, g, dtype, as_stream(stream), dy2->ptr, dy2->ld, dw2);
}

// ---- weight gradient AND bias gradient (= sum of dy over samples and voxels) of a conv behind one entry point: the stem's
// MFMA weight-gradient kernel delivers the bias row from the same pass over dy; elsewhere ru3d_conv3d_wgrad + ru3d_channel_sum
static size_t wgrad_bias_ws_bytes(const ru3d_tensor* dy, const WgradPlan& p) {
    const size_t b = ru3d_reduce_workspace_bytes(dy);
    return p.ws_bytes > b ? p.ws_bytes : b;
}

extern "C" size_t ru3d_conv3d_wgrad_bias_workspace_bytes(const ru3d_tensor* x, const ru3d_tensor* dy, int k, int stride,
                                                         int dtype) {
    RU3D_FWD_F16(dtype, ru3d_conv3d_wgrad_bias_workspace_bytes_f16(x, dy, k, stride, dtype));
    if (!wgrad_shapes_ok(x, dy, k, stride)) return 0;
    return wgrad_bias_ws_bytes(dy, wgrad_plan(make_wgrad(x, dy, k, stride), dtype));
}

extern "C" int ru3d_conv3d_wgrad_bias(const ru3d_tensor* x, const ru3d_tensor* dy, float* dw, float* db, void* ws,
                                      size_t ws_bytes, int k, int stride, int dtype, void* stream) {
    RU3D_FWD_F16(dtype, ru3d_conv3d_wgrad_bias_f16(x, dy, dw, db, ws, ws_bytes, k, stride, dtype, stream));
    Ru3dDeviceGuard dev_guard(stream);
    RU3D_REQUIRE((k == 1 || k == 3) && (stride == 1 || stride == 2), "conv3d_wgrad_bias: k=%d stride=%d unsupported", k, stride);
    RU3D_REQUIRE(wgrad_shapes_ok(x, dy, k, stride) && tensor_ok(x), "conv3d_wgrad_bias: x/dy shape mismatch");
    RU3D_REQUIRE(dw && db && dtype_ok(dtype), "conv3d_wgrad_bias: bad argument");
    const WgradGeom g = make_wgrad(x, dy, k, stride);
    const WgradPlan p = wgrad_plan(g, dtype);
    RU3D_REQUIRE(ws && ws_bytes >= wgrad_bias_ws_bytes(dy, p), "conv3d_wgrad_bias: workspace too small");
    if (p.gives_bias)
        return wgrad_launch(p, x->ptr, dy->ptr, dw, ws, ws_bytes, g, dtype, as_stream(stream), nullptr, 0, nullptr, db);
    int rc = ru3d_conv3d_wgrad(x, dy, dw, ws, ws_bytes, k, stride, dtype, stream);
    if (rc) return rc;
    return ru3d_channel_sum(dy, db, ws, ws_bytes, dtype, stream);
}

// ---- the 1x1x1 head's whole backward (reference network.py:547 fc): dlogits (fp32, as the loss kernel leaves it) -> dx, dW, db
extern "C" int ru3d_head_bwd_supported(const ru3d_tensor* x, const ru3d_tensor* dlogits, const ru3d_tensor* dx, int dtype) {
    RU3D_FWD_F16(dtype, ru3d_head_bwd_supported_f16(x, dlogits, dx, dtype));
    if (!tensor_ok(x) || !tensor_ok(dlogits) || !tensor_ok(dx)) return 0;
    if (x->n != dlogits->n || x->d != dlogits->d || x->h != dlogits->h || x->w != dlogits->w) return 0;
    if (dx->n != x->n || dx->d != x->d || dx->h != x->h || dx->w != x->w || dx->c != x->c) return 0;
    if ((x->ld % 8) || (dx->ld % 8) || ((((uintptr_t)x->ptr) | ((uintptr_t)dx->ptr)) % 16) || (((uintptr_t)dlogits->ptr) % 4)) return 0;
    return head_bwd_eligible(x->c, dlogits->c, dtype) ? 1 : 0;
}

extern "C" size_t ru3d_head_bwd_workspace_bytes(const ru3d_tensor* x, int dtype) {
    RU3D_FWD_F16(dtype, ru3d_head_bwd_workspace_bytes_f16(x, dtype));
    return tensor_ok(x) ? head_bwd_ws_bytes(nvox(x), x->c) : 0;
}

extern "C" int ru3d_head_bwd(const ru3d_tensor* x, const ru3d_tensor* dlogits, const float* weight, int cin_real,
                             const ru3d_tensor* dx, float* dw, float* db, void* ws, size_t ws_bytes, int dtype, void* stream) {
    RU3D_FWD_F16(dtype, ru3d_head_bwd_f16(x, dlogits, weight, cin_real, dx, dw, db, ws, ws_bytes, dtype, stream));
    Ru3dDeviceGuard dev_guard(stream);
    RU3D_REQUIRE(ru3d_head_bwd_supported(x, dlogits, dx, dtype), "head_bwd: shapes have no fused kernel (ask ru3d_head_bwd_supported first)");
    RU3D_REQUIRE(weight && dw && ws && cin_real > 0 && cin_real <= x->c, "head_bwd: bad argument");
    RU3D_REQUIRE(ws_bytes >= head_bwd_ws_bytes(nvox(x), x->c), "head_bwd: workspace too small");
    return head_bwd_launch(x->ptr, x->ld, (const float*)dlogits->ptr, dlogits->ld, weight, cin_real, x->c, dlogits->c, dx->ptr,
                           dx->ld, dw, db, ws, nvox(x), as_stream(stream));
}

// --------------------------------------------------------------------------- ConvTranspose3d(k3,s2,p1) + far pad
static bool convt_shapes_ok(const ru3d_tensor* x, const ru3d_tensor* y) {
    return tensor_ok(x) && tensor_ok(y) && x->n == y->n && y->d == 2 * x->d && y->h == 2 * x->h && y->w == 2 * x->w;
}

extern "C" int ru3d_convtranspose3d_k3s2p1_fwd(const ru3d_tensor* x, const void* w_packed, const float* bias,
                                               const ru3d_tensor* y, int dtype, void* stream) {
    RU3D_FWD_F16(dtype, ru3d_convtranspose3d_k3s2p1_fwd_f16(x, w_packed, bias, y, dtype, stream));
    Ru3dDeviceGuard dev_guard(stream);
    RU3D_REQUIRE(convt_shapes_ok(x, y) && w_packed, "convtranspose3d_fwd: y must have extents 2*x");
    RU3D_REQUIRE(dtype_ok(dtype), "convtranspose3d_fwd: bad dtype");
    return run_conv(x, w_packed, bias, nullptr, y, 3, 2, 1, 0, 1, dtype, dtype, as_stream(stream));
}

static ConvGeom convt_fwd_geom(const ru3d_tensor* x, const ru3d_tensor* y) {
    return conv_geom(x, y, nullptr, 3, 2, 1, 0, 1);
}

// the tile kernel sums the InstanceNorm statistics in its epilogue; *g / *p: the geometry and its plan for the caller
static bool convt_fwd_in_fused(const ru3d_tensor* x, const ru3d_tensor* y, int dtype, ConvGeom* g, ConvDirectPlan* p) {
    if (dtype != RU3D_BF16 || !convt_shapes_ok(x, y) || !mfma_conv_eligible(x->c, y->c, 3, dtype, dtype)) return false;
    *g = convt_fwd_geom(x, y);
    *p = conv_direct_plan(*g);
    return p->tile == S2_TILE_T && conv_direct_tile_ok(*p, *g, x->ptr, nullptr, y->ptr);
}

static size_t convt_fwd_in_ws_bytes(const ru3d_tensor* y, bool fused, const ConvDirectPlan& p) {
    const size_t need = ru3d_reduce_workspace_bytes(y);
    return fused && p.slab_bytes > need ? p.slab_bytes : need;
}

extern "C" size_t ru3d_convtranspose3d_k3s2p1_fwd_in_workspace_bytes(const ru3d_tensor* x, const ru3d_tensor* y, int dtype) {
    RU3D_FWD_F16(dtype, ru3d_convtranspose3d_k3s2p1_fwd_in_workspace_bytes_f16(x, y, dtype));
    if (!tensor_ok(x) || !tensor_ok(y)) return 0;
    ConvGeom g; ConvDirectPlan p;
    return convt_fwd_in_ws_bytes(y, convt_fwd_in_fused(x, y, dtype, &g, &p), p);
}

extern "C" int ru3d_convtranspose3d_k3s2p1_fwd_in(const ru3d_tensor* x, const void* w_packed, const float* bias,
                                                  const ru3d_tensor* y, float* mean, float* scale, void* ws,
                                                  size_t ws_bytes, float eps, int dtype, void* stream) {
    RU3D_FWD_F16(dtype, ru3d_convtranspose3d_k3s2p1_fwd_in_f16(x, w_packed, bias, y, mean, scale, ws, ws_bytes, eps, dtype, stream));
    Ru3dDeviceGuard dev_guard(stream);
    RU3D_REQUIRE(convt_shapes_ok(x, y) && w_packed && mean && scale && ws, "convtranspose3d_fwd_in: bad argument");
    ConvGeom g; ConvDirectPlan p;
    const bool fused = convt_fwd_in_fused(x, y, dtype, &g, &p);
    RU3D_REQUIRE(ws_bytes >= convt_fwd_in_ws_bytes(y, fused, p), "convtranspose3d_fwd_in: workspace too small");
    if (fused) {
        int rc = convt_s2_tile_launch(p, x->ptr, w_packed, bias, nullptr, y->ptr, g, (float*)ws, nullptr, 0, nullptr, as_stream(stream));
        if (rc) return rc;
        return stats_slab_finalize_launch((const float*)ws, p.gx, p.cb, g.N, g.Cout, 1.0 / ((double)g.Do * g.Ho * g.Wo), nullptr, eps,
                                          mean, scale, as_stream(stream));
    }
    int rc = ru3d_convtranspose3d_k3s2p1_fwd(x, w_packed, bias, y, dtype, stream);
    if (rc) return rc;
    return ru3d_instnorm_stats(y, nullptr, mean, scale, ws, ws_bytes, eps, dtype, stream);
}

extern "C" int ru3d_convtranspose3d_k3s2p1_dgrad(const ru3d_tensor* dy, const void* w_packed, const ru3d_tensor* dx,
                                                 int dtype, void* stream) {
    RU3D_FWD_F16(dtype, ru3d_convtranspose3d_k3s2p1_dgrad_f16(dy, w_packed, dx, dtype, stream));
    Ru3dDeviceGuard dev_guard(stream);
    RU3D_REQUIRE(convt_shapes_ok(dx, dy) && w_packed, "convtranspose3d_dgrad: dy must have extents 2*dx");
    RU3D_REQUIRE(dtype_ok(dtype), "convtranspose3d_dgrad: bad dtype");
    // dx[i] = sum_tap dy[2i - 1 + tap] . W[.,.,tap]: a stride-2 gather conv over dy (far planes of dy are zero)
    return run_conv(dy, w_packed, nullptr, nullptr, dx, 3, 2, 0, 0, 0, dtype, dtype, as_stream(stream));
}

static WgradGeom make_convt_wgrad(const ru3d_tensor* x, const ru3d_tensor* dy) {
    // dW[ci][co][tap] = sum_i x[i][ci] dy[2i-1+tap][co]: wgrad of a stride-2 conv whose gathered
    // operand is dy and whose dense operand is x.
    WgradGeom g = make_wgrad(dy, x, 3, 2);
    g.s_o = (int64_t)dy->c * 27;  // "cout" of this view = x.c = module in_channels (outer dim of W[ci][co][tap])
    g.s_i = 27;
    return g;
}

extern "C" size_t ru3d_convtranspose3d_k3s2p1_wgrad_workspace_bytes(const ru3d_tensor* x, const ru3d_tensor* dy,
                                                                    int dtype) {
    RU3D_FWD_F16(dtype, ru3d_convtranspose3d_k3s2p1_wgrad_workspace_bytes_f16(x, dy, dtype));
    if (!convt_shapes_ok(x, dy)) return 0;
    return wgrad_plan(make_convt_wgrad(x, dy), dtype).ws_bytes;
}

extern "C" int ru3d_convtranspose3d_k3s2p1_wgrad(const ru3d_tensor* x, const ru3d_tensor* dy, float* dw, void* ws,
                                                 size_t ws_bytes, int dtype, void* stream) {
    RU3D_FWD_F16(dtype, ru3d_convtranspose3d_k3s2p1_wgrad_f16(x, dy, dw, ws, ws_bytes, dtype, stream));
    Ru3dDeviceGuard dev_guard(stream);
    RU3D_REQUIRE(convt_shapes_ok(x, dy), "convtranspose3d_wgrad: dy must have extents 2*x");
    RU3D_REQUIRE(dw && dtype_ok(dtype), "convtranspose3d_wgrad: bad argument");
    const WgradGeom g = make_convt_wgrad(x, dy);
    return wgrad_launch(wgrad_plan(g, dtype), dy->ptr, x->ptr, dw, ws, ws_bytes, g, dtype, as_stream(stream));
}

}  // namespace RU3D_NS
