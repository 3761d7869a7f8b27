// T5 encoders (T5EncoderModel embedders: sentence-t5, gtr-t5, INSTRUCTOR): the whole-model forward and the sentence-transformers tail
// (mean pooling -> Dense -> Normalize) (include/tt_hip.h, "T5 encoders").  A T5 block is pre-norm and bias-free, and every launch
// of it is one another family has too -- no kernel lives in this file:
//   the schedule           prenorm.h's driver (the one Qwen3 and ModernBERT run on: T5Family below says what is T5's)
//   the norm               varlen.h's rmsnorm_kernel<true>: T5LayerNorm rounds before the weight multiplies
//   the projections        the 16-bit GEMMs (gemm.hip) with a zero bias; the residual adds sit in their epilogues, and so does the
//                          ReLU of the up-projection (TT_EPI_RELU): no pass of its own over [T][F]
//   the attention          tt_attention_relbias (mpnet.hip), unchanged: softmax(q . k / 8 + table).  T5 does not divide by sqrt(d),
//                          so the loader stores the q rows of the fused projection times 8 -- an exponent shift, exact in bf16
//   the gated MLP          varlen.h's gated_act_kernel with the tanh GELU (gelu_new), T5 v1.1 / flan encoders
//
//   the tail               pool_dense.h's kernel with no or one Dense module
//
// Layer schedule (one rounding to bf16 per stored tensor, two inside the norm -- see varlen.h rmsnorm_kernel):
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
#include "pool_dense.h"
#include "prenorm.h"

#include <cmath>

#if TT_F16
#error "t5.hip is bf16 only"
#endif

namespace {

// ---- argument checks -----------------------------------------------------------------------------------------------------------
int check_d_model(int d_model) { return check_hidden("t5", d_model, "d_model"); }

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

VarlenWs t5_plan(const tt_t5_weights* w, int n_rows) {
    const size_t H = (size_t)w->d_model, F = (size_t)w->d_ff, gu = w->mlp_kind == 1 ? 2 * F : 0;   // the gated form's two projections, side by side
    // zeros: the GEMMs' bias operand (the model has none)
    return varlen_plan(n_rows, H, 2 * H, H, H, gu, F, std::max(3 * H, std::max(gu, F)));
}

// what prenorm.h's driver asks of a family
struct T5Family {
    static constexpr QkvForm qkv = QkvForm::SplitV8;
    const tt_t5_weights* w;
    const int32_t* ids;

    PreNormDims dims() const { return {w->d_model, w->d_model, 3 * w->d_model, w->d_ff, w->layers}; }
    int embed(const VarlenBufs& b, int T, hipStream_t st) const { return embed_gather_launch(ids, w->embed, w->vocab, w->d_model, b.ha, T, st); }
    int norm(const uint16_t* in, uint16_t* out, const float* g, const float*, int rows, hipStream_t st) const {
        return rmsnorm_launch<true>(in, out, g, rows, w->d_model, w->eps, st);
    }
    PreNormLayer layer(int l) const {
        const tt_t5_layer_weights& lw = w->layer[l];
        return {lw.ln_attn, lw.qkv_w, lw.o_w, lw.ln_ffn, lw.wi, lw.wo};
    }
    int post_qkv(int, const VarlenBufs&, int, hipStream_t) const { return TT_OK; }
    // (the q rows of qkv_w carry the factor 8 that the kernel's 1 / 8 takes back: T5's unscaled scores)
    int attention(int, const VarlenBufs& b, const PackedSeqs& s, hipStream_t st) const {
        const int H = w->d_model;
        return tt_attention_relbias(b.qkv, 2 * H, 0, H, b.vt, 8 * H, b.ctx, H, s.seq_start, s.seq_len, s.n_seq, s.n_rows, w->heads, 64,
                                    s.max_len, w->bias_table, st);
    }
    const float* final_norm() const { return w->final_norm; }
};

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
    hipStream_t st = (hipStream_t)stream;
    const T5Family fam{w, ids};
    const PackedSeqs s{seq_start, seq_len, n_seq, n_rows, max_len};
    VarlenBufs b;
    if (int rc = varlen_begin(t5_plan(w, n_rows), workspace, n_rows, w->d_model, st, &b)) return rc;
    return w->mlp_kind == 1 ? prenorm_run<GeluTanh>(fam, b, s, hidden_out, st) : prenorm_run<void>(fam, b, s, hidden_out, st);
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
    // LDS: eight rows of d_model + dense_out floats, <= 64 KiB
    return pool_dense_launch(hidden, ld, seq_start, seq_len, n_seq, w->d_model, w->dense_wt ? w->dense_out : 0, 0, w->dense_wt, nullptr,
                             out_f32, out_16, POOL_SB * (1024 + 1024) * sizeof(float), (hipStream_t)stream);
}

}  // extern "C"
