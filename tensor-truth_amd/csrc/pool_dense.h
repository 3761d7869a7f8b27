// The sentence-transformers tail, written once: mean pooling -> Dense (none, one or two; bias-free, identity activation) -> L2
// normalisation, fp32 (t5.hip: tt_t5_pool_dense; gemma.hip: tt_gemma_pool_dense).  The pooling loop is varlen.h's pool_rows_sum.
#pragma once
#include "varlen.h"

namespace {

// ---- the tail: one block of sixteen waves per POOL_SB sequences; a matrix is read once per block, not once per sequence -----------
// The rows live in LDS: buf_a [POOL_SB][wa] (the pooled rows, later the second Dense's outputs; wa = max(H, n2)) and buf_b
// [POOL_SB][n1] (the first Dense's outputs) -- up to 128 KiB with two Dense modules, then one block per CU: its sixteen waves are
// what hides the matrices' load latency.  w1t == nullptr: no Dense (n1 = n2 = 0); w2t == nullptr: one (n2 = 0).
//   pooling  wave v < POOL_SB takes the block's sequence v (varlen.h pool_rows_sum, times 1 / n);
//   Dense    thread t owns the outputs t, t + 1024, ... of all POOL_SB sequences and walks the inputs in ascending order, four per
//            step, over the TRANSPOSED matrix (coalesced rows); the input values are LDS broadcasts;
//   norm     out = v / max(||v||, 1e-12), one wave per sequence; out16 (optional): the same vector in bf16.
// What a sequence gets depends on its own rows only, not on its place in the block or the batch.
constexpr int POOL_SB = 8;
constexpr int POOL_TAIL_THREADS = 1024;

__device__ __forceinline__ void pool_dense_step(const float* __restrict__ in, int in_stride, int K, const float* __restrict__ wt, int N,
                                                float* __restrict__ outp, int out_stride) {
    for (int o = threadIdx.x; o < N; o += POOL_TAIL_THREADS) {
        float acc[POOL_SB];
#pragma unroll
        for (int s = 0; s < POOL_SB; ++s) acc[s] = 0.f;
        for (int i = 0; i < K; i += 4) {
            const float w0 = wt[(size_t)i * N + o], w1 = wt[(size_t)(i + 1) * N + o], w2 = wt[(size_t)(i + 2) * N + o],
                        w3 = wt[(size_t)(i + 3) * N + o];
#pragma unroll
            for (int s = 0; s < POOL_SB; ++s) {
                const float4 x = *reinterpret_cast<const float4*>(in + s * in_stride + i);
                acc[s] += x.x * w0;
                acc[s] += x.y * w1;
                acc[s] += x.z * w2;
                acc[s] += x.w * w3;
            }
        }
#pragma unroll
        for (int s = 0; s < POOL_SB; ++s) outp[s * out_stride + o] = acc[s];
    }
}

__global__ __launch_bounds__(POOL_TAIL_THREADS) void pool_dense_kernel(const uint16_t* __restrict__ hidden, int ld,
                                                                       const int32_t* __restrict__ seq_start,
                                                                       const int32_t* __restrict__ seq_len, int n_seq, int H, int n1,
                                                                       int n2, const float* __restrict__ w1t,
                                                                       const float* __restrict__ w2t, float* __restrict__ out,
                                                                       uint16_t* __restrict__ out16) {
    extern __shared__ float pool_lds[];
    const int wa = H > n2 ? H : n2;
    float* buf_a = pool_lds;
    float* buf_b = pool_lds + POOL_SB * wa;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int b0 = blockIdx.x * POOL_SB;
    for (int slot = wave; slot < POOL_SB; slot += POOL_TAIL_THREADS / 64) {
        const int b = b0 + slot;
        const int s0 = b < n_seq ? seq_start[b] : -1;
        const int n = b < n_seq ? seq_len[b] : 0;
        float acc[2][8];
        pool_rows_sum(hidden, ld, s0, n, H, lane, acc);
        const float inv_n = (s0 >= 0 && n > 0) ? 1.0f / (float)n : 0.f;
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int ch = lane + 64 * j;
            if (ch >= H / 8) continue;
#pragma unroll
            for (int k = 0; k < 8; ++k) buf_a[slot * wa + 8 * ch + k] = acc[j][k] * inv_n;
        }
    }
    __syncthreads();
    const float* vec = buf_a;
    int stride = wa, width = H;
    if (w1t) {   // (uniform over the grid)
        pool_dense_step(buf_a, wa, H, w1t, n1, buf_b, n1);
        __syncthreads();
        vec = buf_b;
        stride = width = n1;
    }
    if (w2t) {   // (uniform over the grid)
        pool_dense_step(buf_b, n1, n1, w2t, n2, buf_a, wa);
        __syncthreads();
        vec = buf_a;
        stride = wa;
        width = n2;
    }
    for (int slot = wave; slot < POOL_SB; slot += POOL_TAIL_THREADS / 64) {
        const int b = b0 + slot;
        if (b >= n_seq) continue;   // (wave-uniform)
        float ss = 0.f;
        for (int o = lane; o < width; o += 64) ss += vec[slot * stride + o] * vec[slot * stride + o];
        const float inv = 1.0f / fmaxf(sqrtf(wave_sum(ss)), 1e-12f);
        for (int o = lane; o < width; o += 64) {
            const float v = vec[slot * stride + o] * inv;
            out[(size_t)b * width + o] = v;
            if (out16) out16[(size_t)b * width + o] = f32_to_bf16_bits(v);
        }
    }
}

// max_lds: the most the entry point's limits allow (the kernel's attribute, set once); the launch itself takes what its widths need
inline int pool_dense_launch(const void* hidden, int ld, const int32_t* seq_start, const int32_t* seq_len, int n_seq, int H, int n1,
                             int n2, const float* w1t, const float* w2t, float* out_f32, void* out_16, size_t max_lds, hipStream_t st) {
    const size_t lds = (size_t)POOL_SB * ((H > n2 ? H : n2) + n1) * sizeof(float);
    TT_SET_MAX_LDS(pool_dense_kernel, max_lds);
    TtProfScope prof(TT_K_ROWOPS, st);
    hipLaunchKernelGGL(pool_dense_kernel, dim3((n_seq + POOL_SB - 1) / POOL_SB), dim3(POOL_TAIL_THREADS), lds, st,
                       (const uint16_t*)hidden, ld, seq_start, seq_len, n_seq, H, n1, n2, w1t, w2t, out_f32, (uint16_t*)out_16);
    TT_CHECK_LAUNCH();
    return TT_OK;
}

}  // namespace
