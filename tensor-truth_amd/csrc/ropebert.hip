// Post-LN BERT encoders with rotary positions (NomicBertModel: nomic-embed-text-v1 / -v1.5; JinaEmbeddingsV3Model: jina-embeddings-v3
// in its transformers format): the whole-model forward and the one kernel that only this family needs (include/tt_hip.h, "RoPE-BERT
// encoders").  The block is the post-LN layer of encoder_api.hip / mpnet.hip without a position table: q and k are rotated
// (rotate-half RoPE, one base for every layer) and the attention is bidirectional over the sequence's own tokens.  Biases are
// optional (NomicBERT has none, Jina has all of them) and the MLP is SwiGLU (mlp_kind 1) or GELU (mlp_kind 0).
//
// Layer schedule (one rounding to the element type per kernel output):
//   qkv  = GEMM(x, Wqkv) + b_qkv                 [T][3H]  Q | K | V, heads of 64              (gemm.hip, TT_EPI_BIAS)
//   qkv  = RoPE(q), RoPE(k) at pos[row]          in place; V copied to the V8 layout vt       (modernbert.hip, tt_rope_v8)
//   ctx  = attention(qkv, vt)                    [T][H]   every key of the sequence           (attention.hip, tt_attention_launch)
//   y    = GEMM(ctx, Wo) + b_o + x               residual fused in the epilogue               (TT_EPI_RESIDUAL)
//   x1   = LayerNorm(y; post_attention_layernorm)                                             (rowops.hip)
//   mlp_kind 1:  gu = GEMM(x1, [Wgate; Wup])     [T][2F]                                      (TT_EPI_BIAS, zero bias)
//                a  = SiLU(gu[:, :F]) * gu[:, F:]                                             (varlen.h gated_act_kernel, the decoder's)
//   mlp_kind 0:  a  = GELU_erf(GEMM(x1, W1) + b1)                                             (TT_EPI_GELU)
//   y    = GEMM(a, Wdown) + b_down + x1                                                       (TT_EPI_RESIDUAL)
//   x    = LayerNorm(y; post_mlp_layernorm)
// with x = LayerNorm(word[ids] + type[0]) before the first layer (varlen.h rb_embed_ln_kernel: the encoder's embedding kernel adds a
// position row, which these models do not have) and no norm behind the last.  A missing bias is the workspace's row of fp32 zeros,
// as on the ModernBERT path.  The attention is the encoder's bidirectional kernel at every length -- the one DESIGN 4.4 builds for
// whole sequences (K / V staged in LDS for four or eight query blocks per workgroup) and the ModernBERT path runs on its global
// layers; a row's arithmetic there does not depend on the batch it travels in.
//
// Compiled twice like the encoder path (common.h TT_F16): bf16 and fp16 (external names with an _f16 suffix, f16_names.h).
#include "varlen.h"

namespace {

// SiLU(gate) * up through varlen.h's gated_act_kernel, as decoder.hip: gu [T][2F] (gate columns, then up columns) -> out [T][F]
struct Silu {
    static __device__ __forceinline__ float f(float x) { return x / (1.0f + expf(-x)); }
};

// (the embedding row op, rb_embed_ln_kernel, is varlen.h's: the JinaBERT path uses it too)

// ---- argument checks -----------------------------------------------------------------------------------------------------------
int check_weights(const tt_ropebert_weights* w) {
    TT_CHECK_ARG(w != nullptr, "null weights");
    if (w->hidden <= 0 || w->hidden % 128 || w->hidden > 1024) {
        tt_set_error("ropebert: hidden=%d must be a multiple of 128 and <= 1024 (the scan's limit)", w->hidden);
        return TT_E_UNSUPPORTED;
    }
    if (w->heads <= 0 || w->hidden != 64 * w->heads) {
        tt_set_error("ropebert: hidden=%d heads=%d: head_dim must be 64", w->hidden, w->heads);
        return TT_E_UNSUPPORTED;
    }
    if (w->mlp_kind != 0 && w->mlp_kind != 1) {
        tt_set_error("ropebert: mlp_kind=%d (0: GELU, 1: SwiGLU)", w->mlp_kind);
        return TT_E_UNSUPPORTED;
    }
    // the GELU MLP's up-projection is F columns wide and the GEMM tiles are 128 columns; SwiGLU's is 2F
    const int fmul = w->mlp_kind == 1 ? 64 : 128;
    if (w->ffn <= 0 || w->ffn % fmul) {
        tt_set_error("ropebert: ffn=%d must be a multiple of %d (mlp_kind %d)", w->ffn, fmul, w->mlp_kind);
        return TT_E_UNSUPPORTED;
    }
    TT_CHECK_ARG(w->layers >= 0 && (w->layers == 0 || w->layer != nullptr), "layer array missing");
    TT_CHECK_ARG(w->word_emb && w->type_emb && w->emb_ln_g && w->emb_ln_b && w->vocab > 0 && w->type_vocab > 0,
                 "embedding tables / embedding LayerNorm missing");
    TT_CHECK_ARG(w->ln_eps > 0.f && w->rope_theta > 0.f, "ln_eps=%g rope_theta=%g", w->ln_eps, w->rope_theta);
    return TT_OK;
}

struct RbWs {
    size_t off_x, off_y, off_x1, off_qkv, off_vt, off_ctx, off_gu, off_act, off_zero, zero_bytes, total;
};

RbWs rb_plan(const tt_ropebert_weights* w, int n_rows) {
    RbWs e{};
    // buffers are sized for a multiple of 256 rows: the attention kernel reads whole key blocks
    const size_t H = (size_t)w->hidden, F = (size_t)w->ffn, T = ((size_t)n_rows + 255) / 256 * 256;
    WsPlanner ws;
    e.off_x = ws.take(T * H * 2);
    e.off_y = ws.take(T * H * 2);
    e.off_x1 = ws.take(T * H * 2);
    e.off_qkv = ws.take(T * 3 * H * 2);
    e.off_vt = ws.take(T * H * 2);
    e.off_ctx = ws.take(T * H * 2);
    e.off_gu = ws.take(w->mlp_kind == 1 ? T * 2 * F * 2 : 0);
    e.off_act = ws.take(T * F * 2);
    e.zero_bytes = std::max(3 * H, 2 * F) * 4;   // the bias operand of a projection without one
    e.off_zero = ws.take(e.zero_bytes);
    e.total = ws.off;
    return e;
}

int rb_layernorm(const uint16_t* in, uint16_t* out, const float* g, const float* b, int rows, int H, float eps, hipStream_t st) {
    TtProfScope prof(TT_K_ROWOPS, st);
    return tt_layernorm_launch(in, out, g, b, rows, H, eps, st);
}

int rb_run(const tt_ropebert_weights* w, const int32_t* ids, const int32_t* pos, const int32_t* seq_start, const int32_t* seq_len,
           int n_seq, int n_rows, int max_len, void* hidden_out, void* workspace, hipStream_t st) {
    const RbWs e = rb_plan(w, n_rows);
    char* ws = (char*)workspace;
    const int H = w->hidden, F = w->ffn, nh = w->heads, T = n_rows;
    uint16_t* xa = (uint16_t*)(ws + e.off_x);
    uint16_t* y = (uint16_t*)(ws + e.off_y);
    uint16_t* x1 = (uint16_t*)(ws + e.off_x1);
    uint16_t* qkv = (uint16_t*)(ws + e.off_qkv);
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
        const tt_ropebert_layer_weights& lw = w->layer[l];
        uint16_t* dst = (l == w->layers - 1) ? (uint16_t*)hidden_out : x;
        GemmParams g = gemm_16(x, lw.qkv_w, lw.qkv_b ? lw.qkv_b : zero, T, 3 * H, H);
        g.C = qkv; g.ldc = 3 * H;
        if (int rc = tt_gemm_launch(g, TT_EPI_BIAS, st)) return rc;
        if (int rc = tt_rope_v8(qkv, 3 * H, pos, T, nh, 64, w->rope_theta, vt, 8 * H, st)) return rc;
        AttnParams a{};
        a.qk = qkv; a.ld_qk = 3 * H; a.q_col0 = 0; a.k_col0 = H; a.vt = vt; a.ldvt = 8 * H;
        a.out = ctx; a.ld_out = H; a.seq_start = seq_start; a.seq_len = seq_len;
        a.n_seq = n_seq; a.heads = nh; a.head_dim = 64; a.max_len = max_len; a.total_rows = T;
        a.scale = 0.125f;
        if (int rc = tt_attention_launch(a, st)) return rc;
        GemmParams go = gemm_16(ctx, lw.o_w, lw.o_b ? lw.o_b : zero, T, H, H);
        go.residual = x; go.ldr = H; go.C = y; go.ldc = H;
        if (int rc = tt_gemm_launch(go, TT_EPI_RESIDUAL, st)) return rc;
        if (int rc = rb_layernorm(y, x1, lw.ln1_g, lw.ln1_b, T, H, w->ln_eps, st)) return rc;
        if (w->mlp_kind == 1) {
            GemmParams g1 = gemm_16(x1, lw.up_w, zero, T, 2 * F, H);
            g1.C = gu; g1.ldc = 2 * F;
            if (int rc = tt_gemm_launch(g1, TT_EPI_BIAS, st)) return rc;
            if (int rc = gated_act_launch<Silu>(gu, act, T, F, st)) return rc;
        } else {
            GemmParams g1 = gemm_16(x1, lw.up_w, lw.up_b ? lw.up_b : zero, T, F, H);
            g1.C = act; g1.ldc = F;
            if (int rc = tt_gemm_launch(g1, TT_EPI_GELU, st)) return rc;
        }
        GemmParams g2 = gemm_16(act, lw.down_w, lw.down_b ? lw.down_b : zero, T, H, F);
        g2.residual = x1; g2.ldr = H; g2.C = y; g2.ldc = H;
        if (int rc = tt_gemm_launch(g2, TT_EPI_RESIDUAL, st)) return rc;
        if (int rc = rb_layernorm(y, dst, lw.ln2_g, lw.ln2_b, T, H, w->ln_eps, st)) return rc;
        x = dst;
    }
    return TT_OK;
}

}  // namespace

extern "C" {

size_t tt_ropebert_workspace_bytes(const tt_ropebert_weights* w, int n_rows) {
    if (!w || n_rows <= 0 || check_weights(w) != TT_OK) return 0;
    return rb_plan(w, n_rows).total;
}

int tt_ropebert_forward(const tt_ropebert_weights* w, const int32_t* ids, const int32_t* pos, const int32_t* type_ids,
                        const int32_t* seq_start, const int32_t* seq_len, int n_seq, int n_rows, int max_len, void* hidden_out,
                        void* workspace, size_t workspace_bytes, void* stream) {
    if (int rc = check_weights(w)) return rc;
    if (int rc = check_packed_forward_args("tt_ropebert_forward", "a RoPE-BERT embedder call", ids, pos, type_ids, seq_start, seq_len,
                                           n_seq, n_rows, max_len, hidden_out, workspace, workspace_bytes, rb_plan(w, n_rows).total))
        return rc;
    for (int l = 0; l < w->layers; ++l) {
        const tt_ropebert_layer_weights& lw = w->layer[l];
        TT_CHECK_ARG(lw.qkv_w && lw.o_w && lw.ln1_g && lw.ln1_b && lw.up_w && lw.down_w && lw.ln2_g && lw.ln2_b,
                     "layer %d has a null weight pointer", l);
        TT_CHECK_ARG(w->mlp_kind == 0 || (!lw.up_b && !lw.down_b), "layer %d: the SwiGLU MLP (mlp_kind 1) takes no biases", l);
    }
    return rb_run(w, ids, pos, seq_start, seq_len, n_seq, n_rows, max_len, hidden_out, workspace, (hipStream_t)stream);
}

}  // extern "C"
