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
#include "postln.h"

namespace {

// (no kernel of its own: the embedding row op, rb_embed_ln_kernel, and the SiLU gate are varlen.h's)

// ---- argument checks -----------------------------------------------------------------------------------------------------------
int check_weights(const tt_ropebert_weights* w) {
    TT_CHECK_ARG(w != nullptr, "null weights");
    if (w->mlp_kind != 0 && w->mlp_kind != 1) {
        tt_set_error("ropebert: mlp_kind=%d (0: GELU, 1: SwiGLU)", w->mlp_kind);
        return TT_E_UNSUPPORTED;
    }
    // the GELU MLP's up-projection is F columns wide and the GEMM tiles are 128 columns; SwiGLU's is 2F
    if (int rc = check_postln_shape("ropebert", w->hidden, w->heads, w->ffn, w->mlp_kind == 1 ? 64 : 128)) return rc;
    TT_CHECK_ARG(w->layers >= 0 && (w->layers == 0 || w->layer != nullptr), "layer array missing");
    TT_CHECK_ARG(w->word_emb && w->type_emb && w->emb_ln_g && w->emb_ln_b && w->vocab > 0 && w->type_vocab > 0,
                 "embedding tables / embedding LayerNorm missing");
    TT_CHECK_ARG(w->ln_eps > 0.f && w->rope_theta > 0.f, "ln_eps=%g rope_theta=%g", w->ln_eps, w->rope_theta);
    return TT_OK;
}

// the zeros are the bias operand of a projection without one: the widest is 3H or 2F
PostLnDims rb_dims(const tt_ropebert_weights* w) {
    return {w->hidden, w->heads, w->ffn, w->layers, w->ln_eps, QkvForm::Packed, w->mlp_kind == 1,
            (size_t)std::max(3 * w->hidden, 2 * w->ffn) * 4, 0};
}

// what postln.h's driver asks of a family
struct RbFamily {
    const tt_ropebert_weights* w;
    const int32_t *ids, *pos;

    int embed(const float*, uint16_t* out, int T, hipStream_t st) const {
        hipLaunchKernelGGL(rb_embed_ln_kernel, dim3((T + 3) / 4), dim3(kRbRowThreads), 0, st, ids, (const uint16_t*)w->word_emb,
                           (const uint16_t*)w->type_emb, w->emb_ln_g, w->emb_ln_b, out, T, w->hidden, w->vocab, w->ln_eps);
        TT_CHECK_LAUNCH();
        return TT_OK;
    }
    PostLnLayer layer(int l, const float* zero) const {
        const tt_ropebert_layer_weights& lw = w->layer[l];
        const auto or_zero = [zero](const float* b) { return b ? b : zero; };
        // (SwiGLU takes no MLP biases: the forward has refused them, so both are the zeros)
        return {lw.qkv_w, or_zero(lw.qkv_b), lw.o_w,    or_zero(lw.o_b),    lw.ln1_g, lw.ln1_b,
                lw.up_w,  or_zero(lw.up_b),  lw.down_w, or_zero(lw.down_b), lw.ln2_g, lw.ln2_b};
    }
    // q and k rotated in place and V copied to the V8 layout, then the encoder's whole-sequence kernel
    int attention(int, const PostLnBufs& b, const PackedSeqs& s, hipStream_t st) const {
        const int H = w->hidden, nh = w->heads;
        if (int rc = tt_rope_v8(b.qkv, 3 * H, pos, s.n_rows, nh, 64, w->rope_theta, b.vt, 8 * H, st)) return rc;
        AttnParams a{};
        a.qk = b.qkv; a.ld_qk = 3 * H; a.q_col0 = 0; a.k_col0 = H; a.vt = b.vt; a.ldvt = 8 * H;
        a.out = b.ctx; a.ld_out = H; a.seq_start = s.seq_start; a.seq_len = s.seq_len;
        a.n_seq = s.n_seq; a.heads = nh; a.head_dim = 64; a.max_len = s.max_len; a.total_rows = s.n_rows;
        a.scale = 0.125f;
        return tt_attention_launch(a, st);
    }
};

}  // namespace

extern "C" {

size_t tt_ropebert_workspace_bytes(const tt_ropebert_weights* w, int n_rows) {
    if (!w || n_rows <= 0 || check_weights(w) != TT_OK) return 0;
    return postln_plan(rb_dims(w), n_rows).total;
}

int tt_ropebert_forward(const tt_ropebert_weights* w, const int32_t* ids, const int32_t* pos, const int32_t* type_ids,
                        const int32_t* seq_start, const int32_t* seq_len, int n_seq, int n_rows, int max_len, void* hidden_out,
                        void* workspace, size_t workspace_bytes, void* stream) {
    if (int rc = check_weights(w)) return rc;
    const PostLnDims d = rb_dims(w);
    if (int rc = check_packed_forward_args("tt_ropebert_forward", "a RoPE-BERT embedder call", ids, pos, type_ids, seq_start, seq_len,
                                           n_seq, n_rows, max_len, hidden_out, workspace, workspace_bytes, postln_plan(d, n_rows).total))
        return rc;
    for (int l = 0; l < w->layers; ++l) {
        const tt_ropebert_layer_weights& lw = w->layer[l];
        TT_CHECK_ARG(lw.qkv_w && lw.o_w && lw.ln1_g && lw.ln1_b && lw.up_w && lw.down_w && lw.ln2_g && lw.ln2_b,
                     "layer %d has a null weight pointer", l);
        TT_CHECK_ARG(w->mlp_kind == 0 || (!lw.up_b && !lw.down_b), "layer %d: the SwiGLU MLP (mlp_kind 1) takes no biases", l);
    }
    const RbFamily fam{w, ids, pos};
    const PackedSeqs s{seq_start, seq_len, n_seq, n_rows, max_len};
    return d.gated ? postln_run<Silu>(d, fam, s, hidden_out, workspace, (hipStream_t)stream)
                   : postln_run<void>(d, fam, s, hidden_out, workspace, (hipStream_t)stream);
}

}  // extern "C"
