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
#include "postln.h"

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
    if (int rc = check_postln_shape("jinabert", w->hidden, w->heads, w->ffn, 128)) return rc;
    TT_CHECK_ARG(w->layers >= 0 && (w->layers == 0 || w->layer != nullptr), "layer array missing");
    TT_CHECK_ARG(w->word_emb && w->type_emb && w->emb_ln_g && w->emb_ln_b && w->vocab > 0 && w->type_vocab > 0,
                 "embedding tables / embedding LayerNorm missing");
    TT_CHECK_ARG(w->alibi_slope_log2 != nullptr, "alibi_slope_log2 missing");
    TT_CHECK_ARG(w->ln_eps > 0.f, "ln_eps=%g", w->ln_eps);
    return TT_OK;
}

// the zeros are the bias operand of the gate projection, which has none
PostLnDims jb_dims(const tt_jinabert_weights* w) {
    return {w->hidden, w->heads, w->ffn, w->layers, w->ln_eps, QkvForm::SplitV8, true, (size_t)2 * w->ffn * 4, 0};
}

// what postln.h's driver asks of a family
struct JbFamily {
    const tt_jinabert_weights* w;
    const int32_t* ids;

    int embed(const float*, uint16_t* out, int T, hipStream_t st) const {
        hipLaunchKernelGGL(rb_embed_ln_kernel, dim3((T + 3) / 4), dim3(kRbRowThreads), 0, st, ids, (const uint16_t*)w->word_emb,
                           (const uint16_t*)w->type_emb, w->emb_ln_g, w->emb_ln_b, out, T, w->hidden, w->vocab, w->ln_eps);
        TT_CHECK_LAUNCH();
        return TT_OK;
    }
    PostLnLayer layer(int l, const float* zero) const {
        const tt_jinabert_layer_weights& lw = w->layer[l];
        return {lw.qkv_w, lw.qkv_b, lw.o_w, lw.o_b, lw.ln1_g, lw.ln1_b, lw.gate_w, zero, lw.down_w, lw.down_b, lw.ln2_g, lw.ln2_b};
    }
    int attention(int, const PostLnBufs& b, const PackedSeqs& s, hipStream_t st) const {
        const int H = w->hidden;
        return alibi_attention_launch(b.qkv, 2 * H, 0, H, b.vt, 8 * H, b.ctx, H, s.seq_start, s.seq_len, s.n_seq, s.n_rows, w->heads,
                                      s.max_len, w->alibi_slope_log2, st);
    }
};

}  // namespace

extern "C" {

size_t tt_jinabert_workspace_bytes(const tt_jinabert_weights* w, int n_rows) {
    if (!w || n_rows <= 0 || check_weights(w) != TT_OK) return 0;
    return postln_plan(jb_dims(w), n_rows).total;
}

int tt_jinabert_forward(const tt_jinabert_weights* w, const int32_t* ids, const int32_t* pos, const int32_t* type_ids,
                        const int32_t* seq_start, const int32_t* seq_len, int n_seq, int n_rows, int max_len, void* hidden_out,
                        void* workspace, size_t workspace_bytes, void* stream) {
    if (int rc = check_weights(w)) return rc;
    const PostLnDims d = jb_dims(w);
    if (int rc = check_packed_forward_args("tt_jinabert_forward", "a JinaBERT embedder call", ids, pos, type_ids, seq_start, seq_len,
                                           n_seq, n_rows, max_len, hidden_out, workspace, workspace_bytes, postln_plan(d, n_rows).total))
        return rc;
    for (int l = 0; l < w->layers; ++l) {
        const tt_jinabert_layer_weights& lw = w->layer[l];
        TT_CHECK_ARG(lw.qkv_w && lw.qkv_b && lw.o_w && lw.o_b && lw.ln1_g && lw.ln1_b && lw.gate_w && lw.down_w && lw.down_b &&
                         lw.ln2_g && lw.ln2_b,
                     "layer %d has a null weight pointer", l);
    }
    // (`pos` is part of the packed-batch contract and is not read: the bias is a function of the row numbers)
    return postln_run<GeluErf>(d, JbFamily{w, ids}, PackedSeqs{seq_start, seq_len, n_seq, n_rows, max_len}, hidden_out, workspace,
                               (hipStream_t)stream);
}

int tt_attention_alibi(const void* qkv, int ld, int q_col0, int k_col0, const void* vt, int ldvt, void* out, int ld_out,
                       const int32_t* seq_start, const int32_t* seq_len, int n_seq, int n_rows, int heads, int head_dim, int max_len,
                       const float* slope_log2, void* stream) {
    if (int rc = check_attention_layout("ALiBi attention", slope_log2 != nullptr, qkv, ld, q_col0, k_col0, vt, ldvt, out, ld_out,
                                        seq_start, seq_len, n_seq, n_rows, heads, head_dim, max_len))
        return rc;
    return alibi_attention_launch((const uint16_t*)qkv, ld, q_col0, k_col0, (const uint16_t*)vt, ldvt, (uint16_t*)out, ld_out, seq_start,
                                  seq_len, n_seq, n_rows, heads, max_len, slope_log2, (hipStream_t)stream);
}

}  // extern "C"
