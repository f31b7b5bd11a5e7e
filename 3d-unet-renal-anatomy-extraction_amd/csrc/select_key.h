// What the radix selects share (prepare.hip: order statistics; topk.hip: top-k statistics inside a loss): the
// order-preserving 32-bit key of a float and the streaming reader of a flat float array.
#pragma once
#include "common.h"

#define PP_THREADS 256

// order-preserving key: a < b as floats <=> key(a) < key(b) as unsigned (-0 just below +0)
__device__ __forceinline__ unsigned pp_key(float x) {
    const unsigned u = __float_as_uint(x);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float pp_unkey(unsigned k) {
    return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k);
}

// f(value) for every element of v[0 .. n): 16-byte loads from the first 16-byte boundary on, the floats before it and
// the last (n - head) % 4 one per lane.  Which lane meets which element depends only on (v, n, grid).  UNROLL: trips of
// the 16-byte loop in flight (1 where f holds wave-wide operations, which the unroller will not duplicate).
template <int UNROLL = 2, typename F>
__device__ __forceinline__ void pp_stream(const float* __restrict__ v, int64_t n, F&& f) {
    const int64_t tid = (int64_t)blockIdx.x * PP_THREADS + threadIdx.x, nthreads = (int64_t)gridDim.x * PP_THREADS;
    int64_t head = (int64_t)(((16 - ((uintptr_t)v & 15)) & 15) >> 2);
    head = head < n ? head : n;
    const int64_t vecs = (n - head) >> 2;
    const float4* p = reinterpret_cast<const float4*>(v + head);
#pragma unroll UNROLL
    for (int64_t i = tid; i < vecs; i += nthreads) {
        const float4 t = p[i];
        f(t.x), f(t.y), f(t.z), f(t.w);
    }
    if (tid < head) f(v[tid]);
    if (tid < n - head - 4 * vecs) f(v[head + 4 * vecs + tid]);
}
