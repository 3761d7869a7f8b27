// JinaBERT encoders (the remote-code architecture behind jinaai/jina-embeddings-v2-small-en / -base-en): the whole-model forward and
// the one kernel that only this family needs (include/tt_hip.h, "JinaBERT encoders").  The block is the post-LN BERT layer of
// encoder_api.hip / mpnet.hip without a position table: every head adds the ALiBi bias -slope_h |query - key| to its scaled
// scores, bidirectional over the sequence's own tokens, and the feed-forward is GEGLU (no bias on the gate projection).
//
// Layer schedule (one rounding to the element type per kernel output):
//   qk, vT = QKV-GEMM(x) + b_qkv                 [T][2H] + the V8 layout [T/8][H][8]          (gemm.hip, TT_EPI_QKV)
//   ctx    = attention(qk, vT; slopes)           [T][H]   softmax(q.k / 8 - slope_h |q - k|)  (varlen.h attention_tile, Alibi)
//   y      = GEMM(ctx, Wo) + b_o + x             residual fused in the epilogue               (TT_EPI_RESIDUAL)
//   x1     = LayerNorm(y; attention.output.LayerNorm)                                         (rowops.hip)
//   gu     = GEMM(x1, Wgate)                     [T][2F]  no bias                             (TT_EPI_BIAS, zero bias)
//   a      = GELU_erf(gu[:, :F]) * gu[:, F:]     [T][F]                                       (varlen.h gated_act_kernel<GeluErf>)
//   y      = GEMM(a, Wdown) + b_down + x1                                                     (TT_EPI_RESIDUAL)
//   x      = LayerNorm(y; mlp.layernorm)
// with x = LayerNorm(word[ids] + type[0]) before the first layer (varlen.h rb_embed_ln_kernel, the RoPE-BERT path's) and no norm
// behind the last.  There is no RoPE launch: the projection's epilogue writes V in the V8 layout itself.  The attention is the
// one-wave tile at every length: the bias is a function of the two row numbers, which the tile has in registers, and a row's
// arithmetic there does not depend on the batch it travels in.
//
// Compiled twice like the encoder path (common.h TT_F16): bf16 and fp16 (external names with an _f16 suffix, f16_names.h).
#include "varlen.h"

namespace {

// ---- bidirectional attention with the ALiBi bias over packed varlen sequences, head_dim 64 -----------------------------------
// One wave per (16-query tile, sequence, head) on varlen.h's tile with the window mask (w >= the longest sequence: every key of the
// sequence) and the Alibi policy; the head's slope is one scalar load.
__global__ __launch_bounds__(64) void jb_attention_kernel(const uint16_t* __restrict__ qkv, int ld, int q_col0, int k_col0,
                                                          const uint16_t* __restrict__ vt, int ldvt, uint16_t* __restrict__ out,
                                                          int ld_out, const int32_t* __restrict__ seq_start,
                                                          const int32_t* __restrict__ seq_len, int n_seq, int n_rows, int w,
                                                          float scale_log2, const float* __restrict__ slope_log2) {
    const int t = blockIdx.x, h = blockIdx.z;
    const Alibi bias{slope_log2[h]};
    for (int b = blockIdx.y; b < n_seq; b += gridDim.y)   // (wave-uniform: every lane takes the same sequences)
        attention_tile<64, true, Alibi>(qkv, ld, q_col0, k_col0, vt, ldvt, out, ld_out, seq_start, seq_len, n_rows, 1, w, scale_log2,
                                        b, h, t, -1, 0, bias);
}

int alibi_attention_launch(const uint16_t* qkv, int ld, int q_col0, int k_col0, const uint16_t* vt, int ldvt, uint16_t* out, int ld_out,
                           const int32_t* seq_start, const int32_t* seq_len, int n_seq, int n_rows, int heads, int max_len,
                           const float* slope_log2, hipStream_t st) {
    const int n_qt = (max_len + 15) / 16;
    const dim3 grid(n_qt, std::min(n_seq, 65535), heads);   // more sequences: each block row takes every 65535th
    const float scale_log2 = 1.4426950408889634f / 8.0f;    // log2(e) / sqrt(64)
    TtProfScope prof(TT_K_ATTENTION, st);
    // w = n_rows: |q - k| < n_rows within a batch, so the window mask keeps every key of the sequence
    hipLaunchKernelGGL(jb_attention_kernel, grid, dim3(64), 0, st, qkv, ld, q_col0, k_col0, vt, ldvt, out, ld_out, seq_start, seq_len,
                       n_seq, n_rows, n_rows, scale_log2, slope_log2);
    TT_CHECK_LAUNCH();
    return TT_OK;
}

// ---- argument checks -----------------------------------------------------------------------------------------------------------
int check_weights(const tt_jinabert_weights* w) {
    TT_CHECK_ARG(w != nullptr, "null weights");
    if (w->hidden <= 0 || w->hidden % 128 || w->hidden > 1024) {
        tt_set_error("jinabert: hidden=%d must be a multiple of 128 and <= 1024 (the scan's limit)", w->hidden);
        return TT_E_UNSUPPORTED;
    }
    if (w->heads <= 0 || w->hidden != 64 * w->heads) {
        tt_set_error("jinabert: hidden=%d heads=%d: head_dim must be 64", w->hidden, w->heads);
        return TT_E_UNSUPPORTED;
    }
    if (w->ffn <= 0 || w->ffn % 128) {
        tt_set_error("jinabert: ffn=%d must be a multiple of 128", w->ffn);
        return TT_E_UNSUPPORTED;
    }
    TT_CHECK_ARG(w->layers >= 0 && (w->layers == 0 || w->layer != nullptr), "layer array missing");
    TT_CHECK_ARG(w->word_emb && w->type_emb && w->emb_ln_g && w->emb_ln_b && w->vocab > 0 && w->type_vocab > 0,
                 "embedding tables / embedding LayerNorm missing");
    TT_CHECK_ARG(w->alibi_slope_log2 != nullptr, "alibi_slope_log2 missing");
    TT_CHECK_ARG(w->ln_eps > 0.f, "ln_eps=%g", w->ln_eps);
    return TT_OK;
}

struct JbWs {
    size_t off_x, off_y, off_x1, off_qk, off_vt, off_ctx, off_gu, off_act, off_zero, zero_bytes, total;
};

JbWs jb_plan(const tt_jinabert_weights* w, int n_rows) {
    JbWs e{};
    // buffers are sized for a multiple of 256 rows: the attention tile reads whole key blocks
    const size_t H = (size_t)w->hidden, F = (size_t)w->ffn, T = ((size_t)n_rows + 255) / 256 * 256;
    WsPlanner ws;
    e.off_x = ws.take(T * H * 2);
    e.off_y = ws.take(T * H * 2);
    e.off_x1 = ws.take(T * H * 2);
    e.off_qk = ws.take(T * 2 * H * 2);
    e.off_vt = ws.take(T * H * 2);
    e.off_ctx = ws.take(T * H * 2);
    e.off_gu = ws.take(T * 2 * F * 2);
    e.off_act = ws.take(T * F * 2);
    e.zero_bytes = 2 * F * 4;        // the bias operand of the gate projection, which has none
    e.off_zero = ws.take(e.zero_bytes);
    e.total = ws.off;
    return e;
}

int jb_layernorm(const uint16_t* in, uint16_t* out, const float* g, const float* b, int rows, int H, float eps, hipStream_t st) {
    TtProfScope prof(TT_K_ROWOPS, st);
    return tt_layernorm_launch(in, out, g, b, rows, H, eps, st);
}

int jb_run(const tt_jinabert_weights* w, const int32_t* ids, const int32_t* seq_start, const int32_t* seq_len, int n_seq, int n_rows,
           int max_len, void* hidden_out, void* workspace, hipStream_t st) {
    const JbWs e = jb_plan(w, n_rows);
    char* ws = (char*)workspace;
    const int H = w->hidden, F = w->ffn, nh = w->heads, T = n_rows;
    uint16_t* xa = (uint16_t*)(ws + e.off_x);
    uint16_t* y = (uint16_t*)(ws + e.off_y);
    uint16_t* x1 = (uint16_t*)(ws + e.off_x1);
    uint16_t* qk = (uint16_t*)(ws + e.off_qk);
    uint16_t* vt = (uint16_t*)(ws + e.off_vt);
    uint16_t* ctx = (uint16_t*)(ws + e.off_ctx);
    uint16_t* gu = (uint16_t*)(ws + e.off_gu);
    uint16_t* act = (uint16_t*)(ws + e.off_act);
    const float* zero = (const float*)(ws + e.off_zero);
    TT_CHECK_HIP(hipMemsetAsync(ws + e.off_zero, 0, e.zero_bytes, st));
    // rows that belong to no sequence are never written by the attention kernel: keep them finite
    TT_CHECK_HIP(hipMemsetAsync(ctx, 0, (size_t)T * H * 2, st));
    uint16_t* x = w->layers == 0 ? (uint16_t*)hidden_out : xa;
    {
        TtProfScope prof(TT_K_ROWOPS, st);
        hipLaunchKernelGGL(rb_embed_ln_kernel, dim3((T + 3) / 4), dim3(kRbRowThreads), 0, st, ids, (const uint16_t*)w->word_emb,
                           (const uint16_t*)w->type_emb, w->emb_ln_g, w->emb_ln_b, x, T, H, w->vocab, w->ln_eps);
        TT_CHECK_LAUNCH();
    }
    for (int l = 0; l < w->layers; ++l) {
        const tt_jinabert_layer_weights& lw = w->layer[l];
        uint16_t* dst = (l == w->layers - 1) ? (uint16_t*)hidden_out : x;
        GemmParams g = gemm_16(x, lw.qkv_w, lw.qkv_b, T, 3 * H, H);
        g.C = qk; g.ldc = 2 * H; g.vt = vt; g.ldvt = 8 * H; g.vt_col0 = 2 * H;
        if (int rc = tt_gemm_launch(g, TT_EPI_QKV, st)) return rc;
        if (int rc = alibi_attention_launch(qk, 2 * H, 0, H, vt, 8 * H, ctx, H, seq_start, seq_len, n_seq, T, nh, max_len,
                                            w->alibi_slope_log2, st))
            return rc;
        GemmParams go = gemm_16(ctx, lw.o_w, lw.o_b, T, H, H);
        go.residual = x; go.ldr = H; go.C = y; go.ldc = H;
        if (int rc = tt_gemm_launch(go, TT_EPI_RESIDUAL, st)) return rc;
        if (int rc = jb_layernorm(y, x1, lw.ln1_g, lw.ln1_b, T, H, w->ln_eps, st)) return rc;
        GemmParams g1 = gemm_16(x1, lw.gate_w, zero, T, 2 * F, H);
        g1.C = gu; g1.ldc = 2 * F;
        if (int rc = tt_gemm_launch(g1, TT_EPI_BIAS, st)) return rc;
        if (int rc = gated_act_launch<GeluErf>(gu, act, T, F, st)) return rc;
        GemmParams g2 = gemm_16(act, lw.down_w, lw.down_b, T, H, F);
        g2.residual = x1; g2.ldr = H; g2.C = y; g2.ldc = H;
        if (int rc = tt_gemm_launch(g2, TT_EPI_RESIDUAL, st)) return rc;
        if (int rc = jb_layernorm(y, dst, lw.ln2_g, lw.ln2_b, T, H, w->ln_eps, st)) return rc;
        x = dst;
    }
    return TT_OK;
}

}  // namespace

extern "C" {

size_t tt_jinabert_workspace_bytes(const tt_jinabert_weights* w, int n_rows) {
    if (!w || n_rows <= 0 || check_weights(w) != TT_OK) return 0;
    return jb_plan(w, n_rows).total;
}

int tt_jinabert_forward(const tt_jinabert_weights* w, const int32_t* ids, const int32_t* pos, const int32_t* type_ids,
                        const int32_t* seq_start, const int32_t* seq_len, int n_seq, int n_rows, int max_len, void* hidden_out,
                        void* workspace, size_t workspace_bytes, void* stream) {
    if (int rc = check_weights(w)) return rc;
    if (int rc = check_packed_forward_args("tt_jinabert_forward", "a JinaBERT embedder call", ids, pos, type_ids, seq_start, seq_len,
                                           n_seq, n_rows, max_len, hidden_out, workspace, workspace_bytes, jb_plan(w, n_rows).total))
        return rc;
    for (int l = 0; l < w->layers; ++l) {
        const tt_jinabert_layer_weights& lw = w->layer[l];
        TT_CHECK_ARG(lw.qkv_w && lw.qkv_b && lw.o_w && lw.o_b && lw.ln1_g && lw.ln1_b && lw.gate_w && lw.down_w && lw.down_b &&
                         lw.ln2_g && lw.ln2_b,
                     "layer %d has a null weight pointer", l);
    }
    // (`pos` is part of the packed-batch contract and is not read: the bias is a function of the row numbers)
    return jb_run(w, ids, seq_start, seq_len, n_seq, n_rows, max_len, hidden_out, workspace, (hipStream_t)stream);
}

int tt_attention_alibi(const void* qkv, int ld, int q_col0, int k_col0, const void* vt, int ldvt, void* out, int ld_out,
                       const int32_t* seq_start, const int32_t* seq_len, int n_seq, int n_rows, int heads, int head_dim, int max_len,
                       const float* slope_log2, void* stream) {
    if (head_dim != 64) {
        tt_set_error("ALiBi attention: head_dim=%d (supported: 64)", head_dim);
        return TT_E_UNSUPPORTED;
    }
    TT_CHECK_ARG(qkv && vt && out && seq_start && seq_len && slope_log2, "null pointer");
    TT_CHECK_ARG(heads > 0 && n_seq > 0 && max_len > 0 && n_rows > 0 && n_rows % 8 == 0 && max_len <= n_rows,
                 "heads=%d n_seq=%d n_rows=%d max_len=%d", heads, n_seq, n_rows, max_len);
    TT_CHECK_ARG(ld % 8 == 0 && q_col0 % 8 == 0 && k_col0 % 8 == 0 && q_col0 >= 0 && k_col0 >= 0 && ld_out % 4 == 0 &&
                     ld >= std::max(q_col0, k_col0) + heads * 64 && ld_out >= heads * 64 && ldvt >= 8 * heads * 64 && ldvt % 8 == 0,
                 "ld=%d q_col0=%d k_col0=%d ld_out=%d ldvt=%d", ld, q_col0, k_col0, ld_out, ldvt);
    return alibi_attention_launch((const uint16_t*)qkv, ld, q_col0, k_col0, (const uint16_t*)vt, ldvt, (uint16_t*)out, ld_out, seq_start,
                                  seq_len, n_seq, n_rows, heads, max_len, slope_log2, (hipStream_t)stream);
}

}  // extern "C"
