// T5 encoders (T5EncoderModel embedders: sentence-t5, gtr-t5, INSTRUCTOR): the whole-model forward, the sentence-transformers tail
// (mean pooling -> Dense -> Normalize) and the two kernels that only this family needs (include/tt_hip.h, "T5 encoders").  A T5 block
// is pre-norm and bias-free; everything but its norm is a launch another family already has:
//   the projections        the 16-bit GEMMs (gemm.hip) with a zero bias; the residual adds sit in their epilogues, and so does the
//                          ReLU of the up-projection (TT_EPI_RELU): no pass of its own over [T][F]
//   the attention          tt_attention_relbias (mpnet.hip), unchanged: softmax(q . k / 8 + table).  T5 does not divide by sqrt(d),
//                          so the loader stores the q rows of the fused projection times 8 -- an exponent shift, exact in bf16
//   the gated MLP          varlen.h's gated_act_kernel with the tanh GELU (gelu_new), T5 v1.1 / flan encoders
//
// Layer schedule (one rounding to bf16 per stored tensor, two inside the norm -- see t5_rmsnorm_kernel):
//   h      = embed[ids]                               [T][H]   before the first layer
//   x      = norm(h; ln_attn)
//   qk, vT = QKV-GEMM(x)                              [T][2H] + the V8 layout [T/8][H][8]
//   ctx    = attention(qk, vT; bias)                  [T][H]   softmax(q . k + bias[h][bucket(key - query)]), bidirectional
//   h1     = GEMM(ctx, Wo) + h                        residual fused in the epilogue
//   x      = norm(h1; ln_ffn)
//   f      = relu(GEMM(x, wi))                        [T][F]   mlp_kind 0;   mlp_kind 1: gu = GEMM(x, [wi_0; wi_1]) [T][2F],
//                                                              f = gelu_new(gu[:, :F]) * gu[:, F:]
//   h      = GEMM(f, wo) + h1
// and after the last layer hidden_out = norm(h; final_norm).  Every row op reads one token row only, so a token's result does not
// depend on how the batch is packed; the attention mixes the rows of one sequence only.
//
// bf16 only: the FFN activations leave fp16's range, so this file is compiled once and has no _f16 twins.
#include "varlen.h"

#include <cmath>

#if TT_F16
#error "t5.hip is bf16 only"
#endif

namespace {

// ---- T5LayerNorm over rows of H <= 1024 elements: one wave per row, four rows per block ------------------------------------------
// out = bf16(bf16(v * rsqrt(mean(v^2) + eps)) * w): fp32 statistics, the normalised value rounded to the element type BEFORE the
// weight multiplies it, as transformers' T5LayerNorm does with 16-bit weights (the decoder path's RMSNorm rounds once, after the
// weight: another rounding point, hence this kernel).  The second product is exact in fp32 when w holds bf16 values.
__global__ __launch_bounds__(256) void t5_rmsnorm_kernel(const uint16_t* __restrict__ in, uint16_t* __restrict__ out,
                                                         const float* __restrict__ g, int rows, int H, float eps) {
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    const uint4* src = reinterpret_cast<const uint4*>(in + (size_t)row * H);
    uint4* dst = reinterpret_cast<uint4*>(out + (size_t)row * H);
    const int nc = H / 8;   // <= 128 chunks of 8 elements: at most two per lane
    uint4 v[2];
    float ss = 0.f;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int c = lane + 64 * j;
        v[j] = c < nc ? src[c] : uint4{0u, 0u, 0u, 0u};
        const uint32_t u[4] = {v[j].x, v[j].y, v[j].z, v[j].w};
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const float a = elo(u[k]), b = ehi(u[k]);
            ss += a * a;
            ss += b * b;
        }
    }
    const float r = rsqrtf(wave_sum(ss) / (float)H + eps);
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int c = lane + 64 * j;
        if (c >= nc) continue;
        const uint32_t u[4] = {v[j].x, v[j].y, v[j].z, v[j].w};
        uint32_t o[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int e = 8 * c + 2 * k;
            const uint32_t n2 = pack_e2(elo(u[k]) * r, ehi(u[k]) * r);   // the first rounding
            o[k] = pack_e2(elo(n2) * g[e], ehi(n2) * g[e + 1]);
        }
        dst[c] = uint4{o[0], o[1], o[2], o[3]};
    }
}

int rmsnorm_launch(const uint16_t* in, uint16_t* out, const float* g, int rows, int H, float eps, hipStream_t st) {
    TtProfScope prof(TT_K_ROWOPS, st);
    hipLaunchKernelGGL(t5_rmsnorm_kernel, dim3((rows + 3) / 4), dim3(256), 0, st, in, out, g, rows, H, eps);
    TT_CHECK_LAUNCH();
    return TT_OK;
}

// gelu_new (transformers NewGELUActivation): 0.5 x (1 + tanh(u)), u = sqrt(2 / pi) (x + 0.044715 x^3), written as
// x / (1 + exp(-2 u)) (1 + tanh(u) = 2 / (1 + exp(-2 u))), fp32.
struct GeluNew {
    static __device__ __forceinline__ float f(float x) {
        const float u = 0.7978845608028654f * (x + 0.044715f * x * x * x);
        return x / (1.0f + expf(-2.0f * u));
    }
};

// ---- the sentence-transformers tail: mean pooling -> Dense (if any) -> L2 normalisation, fp32 --------------------------------------
// One block of sixteen waves per T5_SB sequences: the matrix is read once per block, not once per sequence.  The rows live in LDS:
// buf_a [T5_SB][H] (the pooled rows) and buf_b [T5_SB][N] (the Dense outputs) -- up to 64 KiB.
//   pooling  wave v < T5_SB takes the block's sequence v; a column is summed over the rows seq_start .. seq_start + seq_len - 1 in
//            ascending order (16-byte reads of a row: any row may start a range);
//   Dense    thread t owns the outputs t, t + 1024, ... of all T5_SB sequences and walks the inputs in ascending order over the
//            TRANSPOSED matrix (coalesced rows); the pooled values are LDS broadcasts;
//   norm     out = v / max(||v||, 1e-12), one wave per sequence.
// What a sequence gets depends on its own rows only, not on its place in the block or the batch.
constexpr int T5_SB = 8;
constexpr int T5_TAIL_THREADS = 1024;

__global__ __launch_bounds__(T5_TAIL_THREADS) void t5_pool_dense_kernel(const uint16_t* __restrict__ hidden, int ld,
                                                                        const int32_t* __restrict__ seq_start,
                                                                        const int32_t* __restrict__ seq_len, int n_seq, int H, int N,
                                                                        const float* __restrict__ wt, float* __restrict__ out,
                                                                        uint16_t* __restrict__ out16) {
    extern __shared__ float t5_lds[];
    float* buf_a = t5_lds;
    float* buf_b = t5_lds + T5_SB * H;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int b0 = blockIdx.x * T5_SB;
    for (int slot = wave; slot < T5_SB; slot += T5_TAIL_THREADS / 64) {
        const int b = b0 + slot;
        const int s0 = b < n_seq ? seq_start[b] : -1;
        const int n = b < n_seq ? seq_len[b] : 0;
        // lane owns the 8-element chunks lane, lane + 64 (H <= 1024)
        float acc[2][8];
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int k = 0; k < 8; ++k) acc[j][k] = 0.f;
        if (s0 >= 0) {
            for (int r = 0; r < n; ++r) {
                const uint4* src = reinterpret_cast<const uint4*>(hidden + (size_t)(s0 + r) * ld);
#pragma unroll
                for (int j = 0; j < 2; ++j) {
                    const int ch = lane + 64 * j;
                    if (ch >= H / 8) continue;
                    const uint4 v = src[ch];
                    const uint32_t u[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
                    for (int k = 0; k < 4; ++k) {
                        acc[j][2 * k] += elo(u[k]);
                        acc[j][2 * k + 1] += ehi(u[k]);
                    }
                }
            }
        }
        const float inv_n = (s0 >= 0 && n > 0) ? 1.0f / (float)n : 0.f;
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int ch = lane + 64 * j;
            if (ch >= H / 8) continue;
#pragma unroll
            for (int k = 0; k < 8; ++k) buf_a[slot * H + 8 * ch + k] = acc[j][k] * inv_n;
        }
    }
    __syncthreads();
    const float* vec = buf_a;
    int width = H;
    if (wt) {   // (uniform over the grid)
        for (int o = threadIdx.x; o < N; o += T5_TAIL_THREADS) {
            float acc[T5_SB];
#pragma unroll
            for (int s = 0; s < T5_SB; ++s) acc[s] = 0.f;
            for (int i = 0; i < H; i += 4) {
                const float w0 = wt[(size_t)i * N + o], w1 = wt[(size_t)(i + 1) * N + o], w2 = wt[(size_t)(i + 2) * N + o],
                            w3 = wt[(size_t)(i + 3) * N + o];
#pragma unroll
                for (int s = 0; s < T5_SB; ++s) {
                    const float4 x = *reinterpret_cast<const float4*>(buf_a + s * H + i);
                    acc[s] += x.x * w0;
                    acc[s] += x.y * w1;
                    acc[s] += x.z * w2;
                    acc[s] += x.w * w3;
                }
            }
#pragma unroll
            for (int s = 0; s < T5_SB; ++s) buf_b[s * N + o] = acc[s];
        }
        __syncthreads();
        vec = buf_b;
        width = N;
    }
    for (int slot = wave; slot < T5_SB; slot += T5_TAIL_THREADS / 64) {
        const int b = b0 + slot;
        if (b >= n_seq) continue;   // (wave-uniform)
        float ss = 0.f;
        for (int o = lane; o < width; o += 64) ss += vec[slot * width + o] * vec[slot * width + o];
        const float inv = 1.0f / fmaxf(sqrtf(wave_sum(ss)), 1e-12f);
        for (int o = lane; o < width; o += 64) {
            const float v = vec[slot * width + o] * inv;
            out[(size_t)b * width + o] = v;
            if (out16) out16[(size_t)b * width + o] = f32_to_bf16_bits(v);
        }
    }
}

// ---- argument checks -----------------------------------------------------------------------------------------------------------
int check_d_model(int d_model) {
    if (d_model <= 0 || d_model % 128 || d_model > 1024) {
        tt_set_error("t5: d_model=%d must be a multiple of 128 and <= 1024 (the scan's limit)", d_model);
        return TT_E_UNSUPPORTED;
    }
    return TT_OK;
}

int check_dense(const tt_t5_weights* w) {
    if (!w->dense_wt && w->dense_out == 0) return TT_OK;
    if (!w->dense_wt || w->dense_out <= 0 || w->dense_out % 128 || w->dense_out > 1024) {
        tt_set_error("t5: dense_out=%d%s must be a multiple of 128 and <= 1024 (the scan's limit), with dense_wt", w->dense_out,
                     w->dense_wt ? "" : " (dense_wt NULL)");
        return TT_E_UNSUPPORTED;
    }
    return TT_OK;
}

int check_weights(const tt_t5_weights* w) {
    TT_CHECK_ARG(w != nullptr, "null weights");
    if (int rc = check_d_model(w->d_model)) return rc;
    if (w->d_kv != 64 || w->heads <= 0 || w->heads * 64 != w->d_model) {
        tt_set_error("t5: d_kv=%d num_heads=%d d_model=%d: d_kv must be 64 and num_heads * 64 = d_model", w->d_kv, w->heads, w->d_model);
        return TT_E_UNSUPPORTED;
    }
    if (w->d_ff <= 0 || w->d_ff % 128) {
        tt_set_error("t5: d_ff=%d must be a multiple of 128", w->d_ff);
        return TT_E_UNSUPPORTED;
    }
    if (w->num_buckets != 32) {
        tt_set_error("t5: relative_attention_num_buckets=%d (supported: 32)", w->num_buckets);
        return TT_E_UNSUPPORTED;
    }
    if (w->max_distance != 128) {
        tt_set_error("t5: relative_attention_max_distance=%d (supported: 128)", w->max_distance);
        return TT_E_UNSUPPORTED;
    }
    if (w->mlp_kind != 0 && w->mlp_kind != 1) {
        tt_set_error("t5: mlp_kind=%d (0: relu, 1: gated-gelu)", w->mlp_kind);
        return TT_E_UNSUPPORTED;
    }
    if (int rc = check_dense(w)) return rc;
    TT_CHECK_ARG(w->layers >= 0 && (w->layers == 0 || w->layer != nullptr), "layer array missing");
    TT_CHECK_ARG(w->embed && w->final_norm && w->vocab > 0, "embedding table / final norm missing");
    TT_CHECK_ARG(w->eps > 0.f, "layer_norm_epsilon=%g", w->eps);
    TT_CHECK_ARG(w->rel_bias && w->bias_table, "rel_bias / bias_table missing");
    return TT_OK;
}

struct T5Ws {
    size_t off_ha, off_hb, off_x, off_qk, off_vt, off_ctx, off_gu, off_act, off_zero, zero_bytes, total;
};

T5Ws t5_plan(const tt_t5_weights* w, int n_rows) {
    T5Ws e{};
    // buffers are sized for a multiple of 256 rows: the attention tile reads whole key blocks
    const size_t H = (size_t)w->d_model, F = (size_t)w->d_ff, T = ((size_t)n_rows + 255) / 256 * 256;
    WsPlanner ws;
    e.off_ha = ws.take(T * H * 2);
    e.off_hb = ws.take(T * H * 2);
    e.off_x = ws.take(T * H * 2);
    e.off_qk = ws.take(T * 2 * H * 2);
    e.off_vt = ws.take(H * T * 2);
    e.off_ctx = ws.take(T * H * 2);
    e.off_gu = w->mlp_kind == 1 ? ws.take(T * 2 * F * 2) : 0;   // the gated form's two projections, side by side
    e.off_act = ws.take(T * F * 2);
    // zeros: the GEMMs' bias operand (the model has none)
    e.zero_bytes = std::max(3 * H, (w->mlp_kind == 1 ? 2 : 1) * F) * 4;
    e.off_zero = ws.take(e.zero_bytes);
    e.total = ws.off;
    return e;
}

int t5_run(const tt_t5_weights* w, const int32_t* ids, const int32_t* seq_start, const int32_t* seq_len, int n_seq, int n_rows,
           int max_len, void* hidden_out, void* workspace, hipStream_t st) {
    const T5Ws e = t5_plan(w, n_rows);
    char* ws = (char*)workspace;
    const int H = w->d_model, F = w->d_ff, T = n_rows;
    uint16_t* ha = (uint16_t*)(ws + e.off_ha);
    uint16_t* hb = (uint16_t*)(ws + e.off_hb);
    uint16_t* x = (uint16_t*)(ws + e.off_x);
    uint16_t* qk = (uint16_t*)(ws + e.off_qk);
    uint16_t* vt = (uint16_t*)(ws + e.off_vt);
    uint16_t* ctx = (uint16_t*)(ws + e.off_ctx);
    uint16_t* gu = (uint16_t*)(ws + e.off_gu);
    uint16_t* act = (uint16_t*)(ws + e.off_act);
    const float* zero = (const float*)(ws + e.off_zero);
    TT_CHECK_HIP(hipMemsetAsync(ws + e.off_zero, 0, e.zero_bytes, st));
    // rows that belong to no sequence are never written by the attention kernel: keep them finite
    TT_CHECK_HIP(hipMemsetAsync(ctx, 0, (size_t)T * H * 2, st));
    {
        TtProfScope prof(TT_K_ROWOPS, st);
        hipLaunchKernelGGL(embed_gather_kernel, dim3(T), dim3(128), 0, st, ids, (const uint16_t*)w->embed, w->vocab, H, ha);
        TT_CHECK_LAUNCH();
    }
    for (int l = 0; l < w->layers; ++l) {
        const tt_t5_layer_weights& lw = w->layer[l];
        if (int rc = rmsnorm_launch(ha, x, lw.ln_attn, T, H, w->eps, st)) return rc;
        GemmParams g = gemm_16(x, lw.qkv_w, zero, T, 3 * H, H);
        g.C = qk; g.ldc = 2 * H; g.vt = vt; g.ldvt = 8 * H; g.vt_col0 = 2 * H;
        if (int rc = tt_gemm_launch(g, TT_EPI_QKV, st)) return rc;
        // (the q rows of qkv_w carry the factor 8 that the kernel's 1 / 8 takes back: T5's unscaled scores)
        if (int rc = tt_attention_relbias(qk, 2 * H, 0, H, vt, 8 * H, ctx, H, seq_start, seq_len, n_seq, T, w->heads, 64, max_len,
                                          w->bias_table, st))
            return rc;
        GemmParams go = gemm_16(ctx, lw.o_w, zero, T, H, H);
        go.residual = ha; go.ldr = H; go.C = hb; go.ldc = H;
        if (int rc = tt_gemm_launch(go, TT_EPI_RESIDUAL, st)) return rc;
        if (int rc = rmsnorm_launch(hb, x, lw.ln_ffn, T, H, w->eps, st)) return rc;
        if (w->mlp_kind == 1) {
            GemmParams g1 = gemm_16(x, lw.wi, zero, T, 2 * F, H);
            g1.C = gu; g1.ldc = 2 * F;
            if (int rc = tt_gemm_launch(g1, TT_EPI_BIAS, st)) return rc;
            if (int rc = gated_act_launch<GeluNew>(gu, act, T, F, st)) return rc;
        } else {
            GemmParams g1 = gemm_16(x, lw.wi, zero, T, F, H);
            g1.C = act; g1.ldc = F;
            if (int rc = tt_gemm_launch(g1, TT_EPI_RELU, st)) return rc;
        }
        GemmParams g2 = gemm_16(act, lw.wo, zero, T, H, F);
        g2.residual = hb; g2.ldr = H; g2.C = ha; g2.ldc = H;
        if (int rc = tt_gemm_launch(g2, TT_EPI_RESIDUAL, st)) return rc;
    }
    return rmsnorm_launch(ha, (uint16_t*)hidden_out, w->final_norm, T, H, w->eps, st);
}

}  // namespace

extern "C" {

size_t tt_t5_workspace_bytes(const tt_t5_weights* w, int n_rows) {
    if (!w || n_rows <= 0 || check_weights(w) != TT_OK) return 0;
    return t5_plan(w, n_rows).total;
}

int tt_t5_forward(const tt_t5_weights* w, const int32_t* ids, const int32_t* pos, const int32_t* type_ids, const int32_t* seq_start,
                  const int32_t* seq_len, int n_seq, int n_rows, int max_len, void* hidden_out, void* workspace, size_t workspace_bytes,
                  void* stream) {
    if (int rc = check_weights(w)) return rc;
    if (int rc = check_packed_forward_args("tt_t5_forward", "T5", ids, pos, type_ids, seq_start, seq_len, n_seq, n_rows, max_len,
                                           hidden_out, workspace, workspace_bytes, t5_plan(w, n_rows).total))
        return rc;
    if (max_len > 512) {
        tt_set_error("t5: max_len=%d: sequences of up to 512 tokens", max_len);
        return TT_E_UNSUPPORTED;
    }
    for (int l = 0; l < w->layers; ++l) {
        const tt_t5_layer_weights& lw = w->layer[l];
        TT_CHECK_ARG(lw.ln_attn && lw.qkv_w && lw.o_w && lw.ln_ffn && lw.wi && lw.wo, "layer %d has a null weight pointer", l);
    }
    return t5_run(w, ids, seq_start, seq_len, n_seq, n_rows, max_len, hidden_out, workspace, (hipStream_t)stream);
}

int tt_t5_pool_dense(const tt_t5_weights* w, const void* hidden, int ld, const int32_t* seq_start, const int32_t* seq_len, int n_seq,
                     float* out_f32, void* out_16, void* stream) {
    TT_CHECK_ARG(w != nullptr, "null weights");
    if (int rc = check_d_model(w->d_model)) return rc;
    if (int rc = check_dense(w)) return rc;
    TT_CHECK_ARG(n_seq >= 0, "n_seq=%d", n_seq);
    if (n_seq == 0) return TT_OK;
    TT_CHECK_ARG(hidden && seq_start && seq_len && out_f32, "null pointer");
    TT_CHECK_ARG(ld >= w->d_model && ld % 8 == 0 && ((uintptr_t)hidden % 16) == 0, "d_model=%d ld=%d (16-byte aligned rows)", w->d_model,
                 ld);
    hipStream_t st = (hipStream_t)stream;
    const int N = w->dense_wt ? w->dense_out : 0;
    const size_t lds = (size_t)T5_SB * (w->d_model + N) * sizeof(float);   // <= 64 KiB
    TT_SET_MAX_LDS(t5_pool_dense_kernel, T5_SB * (1024 + 1024) * sizeof(float));
    TtProfScope prof(TT_K_ROWOPS, st);
    hipLaunchKernelGGL(t5_pool_dense_kernel, dim3((n_seq + T5_SB - 1) / T5_SB), dim3(T5_TAIL_THREADS), lds, st, (const uint16_t*)hidden,
                       ld, seq_start, seq_len, n_seq, w->d_model, N, w->dense_wt, out_f32, (uint16_t*)out_16);
    TT_CHECK_LAUNCH();
    return TT_OK;
}

}  // extern "C"
