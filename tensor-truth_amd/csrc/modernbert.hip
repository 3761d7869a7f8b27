// ModernBERT encoders (ModernBertModel embedders, ModernBertForSequenceClassification cross-encoders): the whole-model forward, the
// classification head and the kernels that only this family needs (include/tt_hip.h, "ModernBERT encoders").  The projections run
// on the encoder's GEMMs (gemm.hip), the LayerNorms on the encoder's row op (rowops.hip) with a zero beta, and the global layers'
// attention on the encoder's bidirectional kernel (attention.hip).
//
// Layer schedule (pre-norm block, no biases; one rounding to the element type per kernel output):
//   x    = LayerNorm(h) * g_attn                         [T][H]   (layer 0 has no attn_norm: x = h)
//   qkv  = GEMM(x, Wqkv)                                 [T][3H]  Q | K | V, heads of 64
//   qkv  = RoPE(q), RoPE(k) with the layer's base        in place; V copied to the V8 layout vt
//   ctx  = attention(qkv, vt)                            [T][H]   bidirectional; a sliding layer keeps |q - k| <= local_attention / 2
//                                                                 (the shared tile, varlen.h attention_tile, with the window mask)
//   h1   = GEMM(ctx, Wo) + h                             residual fused in the epilogue
//   x    = LayerNorm(h1) * g_mlp
//   gu   = GEMM(x, Wi)                                   [T][2F]  "input" columns, then "gate" columns
//   a    = GELU_erf(gu[:, :F]) * gu[:, F:]               [T][F]
//   h    = GEMM(a, Wo_mlp) + h1
// with h = LayerNorm(tok_embeddings[ids]) * g_emb before the first layer and out = LayerNorm(h) * g_final after the last.  Every
// row op reads one token row only, so a token's result does not depend on how the batch is packed; the attention mixes the rows of
// one sequence only.  The schedule itself is prenorm.h's (the driver Qwen3 and T5 run on too: MbFamily below says what is
// ModernBERT's); the attention tile and its windowed wrapper, the embedding gather, the gated-activation kernel, the workspace plan
// and the batch-argument checks are varlen.h's, and so is the head's pooling loop.
//
// Compiled twice like the encoder path (common.h TT_F16): bf16 and fp16 (external names with an _f16 suffix, f16_names.h).
#include "prenorm.h"

#include <cmath>

namespace {

// (the exact-erf GELU gate, GeluErf, is varlen.h's: the JinaBERT path uses it too)

// ---- rotate-half RoPE of the q and k heads with base theta, in place; V heads copied to the V8 layout ------------------------
// One block per token row, one wave per head at a time; heads of 64: lane i < 32 holds the pair (i, i + 32).
//   inv_freq[i] = theta^(-2 i / 64), angle = pos * inv_freq[i] (fp32, as transformers' default rotary embedding)
//   out[i] = x[i] cos - x[i + 32] sin,  out[i + 32] = x[i + 32] cos + x[i] sin
// inv_freq comes from the host, rounded once from double (a kernel argument: 32 floats): at position 8191 an error of a few ulp in
// it, as a device powf may leave, is an angle error of 1e-3 rad -- more than fp16's unit roundoff.
// Lane i reads inv[i] with one global_load_dword from the kernel-argument segment (no scratch copy: checked in the disassembly).
struct MbRopeFreq {
    float inv[32];
};
__global__ __launch_bounds__(256) void mb_rope_kernel(uint16_t* __restrict__ qkv, int ld, const int32_t* __restrict__ pos, int heads,
                                                      MbRopeFreq freq, uint16_t* __restrict__ vt, int ldvt) {
    constexpr int D = 64, half = 32;
    const int row = blockIdx.x;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const float p = (float)pos[row];
    uint16_t* r = qkv + (size_t)row * ld;
    float c = 1.f, s = 0.f;
    if (lane < half) sincosf(p * freq.inv[lane], &s, &c);
    for (int h = wave; h < 3 * heads; h += 4) {
        uint16_t* x = r + (size_t)h * D;
        if (h >= 2 * heads) {   // V head: vt[(row / 8) * ldvt + feature * 8 + row % 8]
            const size_t f0 = (size_t)(h - 2 * heads) * D;
            vt[(size_t)(row >> 3) * ldvt + (f0 + lane) * 8 + (row & 7)] = x[lane];
            continue;
        }
        if (lane < half) {
            const float a = ebits_to_f32(x[lane]), b = ebits_to_f32(x[lane + half]);
            x[lane] = f32_to_ebits(a * c - b * s);
            x[lane + half] = f32_to_ebits(b * c + a * s);
        }
    }
}

// ---- classification head: pooling -> head.dense -> GELU -> head.norm -> classifier -> sigmoid, fp32 ---------------------------
// One wave (one block) per sequence.  The pooled row (the first token's, or the mean over the sequence's tokens summed in ascending
// order) goes to LDS; lane l owns the dense outputs l, l + 64, ... and walks the inputs in ascending order over the TRANSPOSED
// matrix (coalesced rows), so a sequence's logit does not depend on the batch it travels in.
__global__ __launch_bounds__(64) void mb_head_kernel(const uint16_t* __restrict__ hidden, int ld, const int32_t* __restrict__ seq_start,
                                                     const int32_t* __restrict__ seq_len, int H, int pooling,
                                                     const float* __restrict__ dense_wt, const float* __restrict__ norm_g,
                                                     const float* __restrict__ cls_w, const float* __restrict__ cls_b, float eps,
                                                     float* __restrict__ scores, float* __restrict__ logits) {
    __shared__ float pooled[1024];
    const int b = blockIdx.x, lane = threadIdx.x;
    const int s0 = seq_start[b];
    const int n = pooling ? seq_len[b] : 1;
    const bool ok = s0 >= 0 && n > 0;
    // pooled row: lane owns the 8-element chunks lane, lane + 64 (H <= 1024)
    float acc[2][8];
    pool_rows_sum(hidden, ld, s0, n, H, lane, acc);
    const float inv_n = ok ? 1.0f / (float)n : 0.f;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int ch = lane + 64 * j;
        if (ch >= H / 8) continue;
#pragma unroll
        for (int k = 0; k < 8; ++k) pooled[8 * ch + k] = pooling ? acc[j][k] * inv_n : acc[j][k];
    }
    __syncthreads();
    // dense (no bias): y[o] = sum_i pooled[i] * Wt[i][o], o = lane + 64 jj
    float y[16];
#pragma unroll
    for (int jj = 0; jj < 16; ++jj) y[jj] = 0.f;
    const int no = H / 64;   // outputs per lane (H a multiple of 64)
    for (int i = 0; i < H; ++i) {
        const float p = pooled[i];
        const float* wr = dense_wt + (size_t)i * H + lane;
#pragma unroll
        for (int jj = 0; jj < 16; ++jj)
            if (jj < no) y[jj] += p * wr[64 * jj];
    }
    // GELU (libm erf: a few hundred rows per call), then LayerNorm (weight only) in two passes
    float sum = 0.f;
#pragma unroll
    for (int jj = 0; jj < 16; ++jj) {
        if (jj < no) {
            y[jj] = 0.5f * y[jj] * (1.0f + erff(y[jj] * 0.70710678118654752f));
            sum += y[jj];
        }
    }
    const float mean = wave_sum(sum) / (float)H;
    float var = 0.f;
#pragma unroll
    for (int jj = 0; jj < 16; ++jj) {
        if (jj < no) {
            const float d = y[jj] - mean;
            var += d * d;
        }
    }
    const float rstd = rsqrtf(wave_sum(var) / (float)H + eps);
    float dot = 0.f;
#pragma unroll
    for (int jj = 0; jj < 16; ++jj) {
        if (jj < no) {
            const int o = lane + 64 * jj;
            dot += (y[jj] - mean) * rstd * norm_g[o] * cls_w[o];
        }
    }
    dot = wave_sum(dot) + cls_b[0];
    if (lane == 0) {
        scores[b] = 1.0f / (1.0f + expf(-dot));
        if (logits) logits[b] = dot;
    }
}

// ---- argument checks -----------------------------------------------------------------------------------------------------------
int check_shape(int hidden, int heads, int ffn) {
    if (int rc = check_hidden("modernbert", hidden)) return rc;
    if (heads <= 0 || hidden != 64 * heads) {
        tt_set_error("modernbert: hidden=%d heads=%d: head_dim must be 64", hidden, heads);
        return TT_E_UNSUPPORTED;
    }
    if (ffn <= 0 || ffn % 64) {
        tt_set_error("modernbert: ffn=%d must be a multiple of 64", ffn);
        return TT_E_UNSUPPORTED;
    }
    return TT_OK;
}

int check_weights(const tt_modernbert_weights* w) {
    TT_CHECK_ARG(w != nullptr, "null weights");
    if (int rc = check_shape(w->hidden, w->heads, w->ffn)) return rc;
    TT_CHECK_ARG(w->layers >= 0 && (w->layers == 0 || w->layer != nullptr), "layer array missing");
    TT_CHECK_ARG(w->embed && w->emb_norm && w->final_norm && w->vocab > 0, "embedding table / embedding norm / final norm missing");
    TT_CHECK_ARG(w->norm_eps > 0.f && w->global_rope_theta > 0.f && w->local_rope_theta > 0.f && w->local_attention >= 0,
                 "norm_eps=%g global_rope_theta=%g local_rope_theta=%g local_attention=%d", w->norm_eps, w->global_rope_theta,
                 w->local_rope_theta, w->local_attention);
    return TT_OK;
}

VarlenWs mb_plan(const tt_modernbert_weights* w, int n_rows) {
    const size_t H = (size_t)w->hidden, F = (size_t)w->ffn;
    // zeros: the GEMMs' bias operand and the LayerNorms' beta (the model has neither)
    return varlen_plan(n_rows, H, 3 * H, H, H, 2 * F, F, std::max(3 * H, 2 * F));
}

int rope_launch(uint16_t* qkv, int ld, const int32_t* pos, int rows, int heads, float theta, uint16_t* vt, int ldvt, hipStream_t st) {
    MbRopeFreq freq;
    for (int i = 0; i < 32; ++i) freq.inv[i] = (float)pow((double)theta, -(double)(2 * i) / 64.0);
    TtProfScope prof(TT_K_ROWOPS, st);
    hipLaunchKernelGGL(mb_rope_kernel, dim3(rows), dim3(256), 0, st, qkv, ld, pos, heads, freq, vt, ldvt);
    TT_CHECK_LAUNCH();
    return TT_OK;
}

// what prenorm.h's driver asks of a family
struct MbFamily {
    static constexpr QkvForm qkv = QkvForm::Packed;
    const tt_modernbert_weights* w;
    const int32_t *ids, *pos;

    PreNormDims dims() const { return {w->hidden, w->hidden, 3 * w->hidden, w->ffn, w->layers}; }
    // the LayerNorms are the encoder's row op (rowops.hip) with a zero beta
    int norm(const uint16_t* in, uint16_t* out, const float* g, const float* zero, int rows, hipStream_t st) const {
        TtProfScope prof(TT_K_ROWOPS, st);
        return tt_layernorm_launch(in, out, g, zero, rows, w->hidden, w->norm_eps, st);
    }
    int embed(const VarlenBufs& b, int T, hipStream_t st) const {
        if (int rc = embed_gather_launch(ids, w->embed, w->vocab, w->hidden, b.hb, T, st)) return rc;
        return norm(b.hb, b.ha, w->emb_norm, b.zero, T, st);
    }
    PreNormLayer layer(int l) const {
        const tt_modernbert_layer_weights& lw = w->layer[l];
        return {lw.attn_norm, lw.qkv_w, lw.o_w, lw.mlp_norm, lw.wi_w, lw.wo_w};
    }
    int post_qkv(int l, const VarlenBufs& b, int T, hipStream_t st) const {
        return rope_launch(b.qkv, 3 * w->hidden, pos, T, w->heads, w->layer[l].sliding ? w->local_rope_theta : w->global_rope_theta, b.vt,
                           8 * w->hidden, st);
    }
    int attention(int l, const VarlenBufs& b, const PackedSeqs& s, hipStream_t st) const {
        const int H = w->hidden;
        if (w->layer[l].sliding)
            return window_attention_launch<64>(b.qkv, 3 * H, 0, H, b.vt, 8 * H, b.ctx, H, s.seq_start, s.seq_len, s.n_seq, s.n_rows,
                                               w->heads, w->heads, s.max_len, w->local_attention / 2, st);
        // global layers: the encoder's bidirectional kernel (64-wide heads, the same Q / K rows and V8 layout)
        AttnParams a{};
        a.qk = b.qkv; a.ld_qk = 3 * H; a.q_col0 = 0; a.k_col0 = H; a.vt = b.vt; a.ldvt = 8 * H;
        a.out = b.ctx; a.ld_out = H; a.seq_start = s.seq_start; a.seq_len = s.seq_len;
        a.n_seq = s.n_seq; a.heads = w->heads; a.head_dim = 64; a.max_len = s.max_len; a.total_rows = s.n_rows;
        a.scale = 0.125f;
        return tt_attention_launch(a, st);
    }
    const float* final_norm() const { return w->final_norm; }
};

}  // namespace

extern "C" {

size_t tt_modernbert_workspace_bytes(const tt_modernbert_weights* w, int n_rows) {
    if (!w || n_rows <= 0 || check_weights(w) != TT_OK) return 0;
    return mb_plan(w, n_rows).total;
}

int tt_modernbert_forward(const tt_modernbert_weights* w, const int32_t* ids, const int32_t* pos, const int32_t* type_ids,
                          const int32_t* seq_start, const int32_t* seq_len, int n_seq, int n_rows, int max_len, void* hidden_out,
                          void* workspace, size_t workspace_bytes, void* stream) {
    if (int rc = check_weights(w)) return rc;
    if (int rc = check_packed_forward_args("tt_modernbert_forward", "ModernBERT", ids, pos, type_ids, seq_start, seq_len, n_seq, n_rows,
                                           max_len, hidden_out, workspace, workspace_bytes, mb_plan(w, n_rows).total))
        return rc;
    for (int l = 0; l < w->layers; ++l) {
        const tt_modernbert_layer_weights& lw = w->layer[l];
        TT_CHECK_ARG(lw.qkv_w && lw.o_w && lw.mlp_norm && lw.wi_w && lw.wo_w, "layer %d has a null weight pointer", l);
    }
    hipStream_t st = (hipStream_t)stream;
    VarlenBufs b;
    if (int rc = varlen_begin(mb_plan(w, n_rows), workspace, n_rows, w->hidden, st, &b)) return rc;
    return prenorm_run<GeluErf>(MbFamily{w, ids, pos}, b, PackedSeqs{seq_start, seq_len, n_seq, n_rows, max_len}, hidden_out, st);
}

int tt_modernbert_head(const tt_modernbert_weights* w, const void* hidden, int ld, const int32_t* seq_start, const int32_t* seq_len,
                       int n_seq, int pooling, float* scores, float* logits, void* stream) {
    TT_CHECK_ARG(w != nullptr, "null weights");
    if (int rc = check_shape(w->hidden, w->heads, w->ffn)) return rc;
    TT_CHECK_ARG(n_seq > 0, "n_seq=%d", n_seq);
    TT_CHECK_ARG(pooling == 0 || pooling == 1, "pooling=%d (0: first token, 1: mean)", pooling);
    TT_CHECK_ARG(hidden && seq_start && scores && (pooling == 0 || seq_len), "null pointer");
    TT_CHECK_ARG(w->head_dense_wt && w->head_norm && w->cls_w && w->cls_b, "these weights carry no classification head");
    TT_CHECK_ARG(ld >= w->hidden && ld % 8 == 0 && ((uintptr_t)hidden % 16) == 0, "hidden=%d ld=%d (16-byte aligned rows)", w->hidden, ld);
    TT_CHECK_ARG(w->norm_eps > 0.f, "norm_eps=%g", w->norm_eps);
    hipStream_t st = (hipStream_t)stream;
    TtProfScope prof(TT_K_ROWOPS, st);
    hipLaunchKernelGGL(mb_head_kernel, dim3(n_seq), dim3(64), 0, st, (const uint16_t*)hidden, ld, seq_start, seq_len, w->hidden, pooling,
                       w->head_dense_wt, w->head_norm, w->cls_w, w->cls_b, w->norm_eps, scores, logits);
    TT_CHECK_LAUNCH();
    return TT_OK;
}

int tt_rope_v8(void* qkv, int ld, const int32_t* pos, int n_rows, int heads, int head_dim, float rope_theta, void* vt, int ldvt,
               void* stream) {
    if (head_dim != 64) {
        tt_set_error("rope: head_dim=%d (supported: 64)", head_dim);
        return TT_E_UNSUPPORTED;
    }
    TT_CHECK_ARG(qkv && pos && vt, "null pointer");
    TT_CHECK_ARG(heads > 0 && n_rows > 0 && n_rows % 8 == 0 && ld >= 3 * heads * 64 && ldvt >= 8 * heads * 64,
                 "heads=%d n_rows=%d ld=%d ldvt=%d", heads, n_rows, ld, ldvt);
    TT_CHECK_ARG(rope_theta > 0.f, "rope_theta=%g", rope_theta);
    return rope_launch((uint16_t*)qkv, ld, pos, n_rows, heads, rope_theta, (uint16_t*)vt, ldvt, (hipStream_t)stream);
}

int tt_attention_window(const void* qkv, int ld, int q_col0, int k_col0, const void* vt, int ldvt, void* out, int ld_out,
                        const int32_t* seq_start, const int32_t* seq_len, int n_seq, int n_rows, int heads, int head_dim,
                        int max_len, int window, void* stream) {
    if (int rc = check_attention_layout("windowed attention", true, qkv, ld, q_col0, k_col0, vt, ldvt, out, ld_out, seq_start, seq_len,
                                        n_seq, n_rows, heads, head_dim, max_len))
        return rc;
    return window_attention_launch<64>((const uint16_t*)qkv, ld, q_col0, k_col0, (const uint16_t*)vt, ldvt, (uint16_t*)out, ld_out,
                                       seq_start, seq_len, n_seq, n_rows, heads, heads, max_len, window, (hipStream_t)stream);
}

}  // extern "C"
