// MPNet encoders (MPNetModel embedders: all-mpnet-base-v2, multi-qa-mpnet-base-*): the whole-model forward and the one kernel that
// only this family needs (include/tt_hip.h, "MPNet encoders").  MPNet is the post-LN BERT block of encoder_api.hip with a learned
// relative-position bias added to every layer's attention scores, one [32 buckets][heads] table for all layers.  The embedding +
// LayerNorm, the projections and the LayerNorms are the encoder's own launches (rowops.hip, gemm.hip); the attention is the shared
// one-wave tile (varlen.h attention_tile) with the RelBias policy.
//
// Layer schedule (postln.h's driver: QkvForm::SplitV8, the GELU MLP; one rounding to the element type per fused kernel output):
//   qk, vT = QKV-GEMM(x)                       [T][2H] + the V8 layout [T/8][H][8]
//   ctx    = attention(qk, vT; bias)           [T][H]   softmax(q.k / 8 + bias[h][bucket(key - query)]), bidirectional
//   y      = GEMM(ctx, Wo) + bo + x            residual fused in the epilogue
//   x1     = LayerNorm(y)
//   f      = GELU(GEMM(x1, W1) + b1)           [T][F]
//   y      = GEMM(f, W2) + b2 + x1
//   x      = LayerNorm(y)
// with x = LayerNorm(word[ids] + position[pos]) before the first layer (no token types: the embedding kernel's type row is a row of
// zeros in the workspace).  The bias of a distance is a lookup: bias_table[h][clamp(key - query, -R, R) + R], R = 128, built by the
// host from the checkpoint's table and the bucket function and already multiplied by log2(e) -- every distance beyond +-R shares
// the last bucket of its side (max_distance 128), so the clamp is exact.  No logarithm is evaluated on the device.
//
// Compiled twice like the encoder path (common.h TT_F16): bf16 and fp16 (external names with an _f16 suffix, f16_names.h).
#include "postln.h"

namespace {

// ---- bidirectional attention with the relative-position bias over packed varlen sequences, head_dim 64 -------------------------
// One wave per (16-query tile, sequence, head) on varlen.h's tile with the window mask (w >= the longest sequence: every key of the
// sequence) and the RelBias policy; the head's table is staged in LDS once per workgroup, before the walk over the sequences.
__global__ __launch_bounds__(64) void mp_attention_kernel(const uint16_t* __restrict__ qkv, int ld, int q_col0, int k_col0,
                                                          const uint16_t* __restrict__ vt, int ldvt, uint16_t* __restrict__ out,
                                                          int ld_out, const int32_t* __restrict__ seq_start,
                                                          const int32_t* __restrict__ seq_len, int n_seq, int n_rows, int w,
                                                          float scale_log2, const float* __restrict__ tbl) {
    __shared__ float bias_lds[RelBias::LDS_FLOATS];
    const int t = blockIdx.x, h = blockIdx.z;
    relbias_stage(tbl, h, bias_lds);
    for (int b = blockIdx.y; b < n_seq; b += gridDim.y)   // (wave-uniform: every lane takes the same sequences)
        attention_tile<64, true, RelBias>(qkv, ld, q_col0, k_col0, vt, ldvt, out, ld_out, seq_start, seq_len, n_rows, 1, w, scale_log2,
                                          b, h, t, -1, 0, RelBias{bias_lds});
}

int relbias_attention_launch(const uint16_t* qkv, int ld, int q_col0, int k_col0, const uint16_t* vt, int ldvt, uint16_t* out, int ld_out,
                             const int32_t* seq_start, const int32_t* seq_len, int n_seq, int n_rows, int heads, int max_len,
                             const float* tbl, hipStream_t st) {
    const int n_qt = (max_len + 15) / 16;
    const dim3 grid(n_qt, std::min(n_seq, 65535), heads);   // more sequences: each block row takes every 65535th
    const float scale_log2 = 1.4426950408889634f / 8.0f;    // log2(e) / sqrt(64)
    TtProfScope prof(TT_K_ATTENTION, st);
    // w = n_rows: |q - k| < n_rows within a batch, so the window mask keeps every key of the sequence
    hipLaunchKernelGGL(mp_attention_kernel, grid, dim3(64), 0, st, qkv, ld, q_col0, k_col0, vt, ldvt, out, ld_out, seq_start, seq_len,
                       n_seq, n_rows, n_rows, scale_log2, tbl);
    TT_CHECK_LAUNCH();
    return TT_OK;
}

// ---- argument checks -----------------------------------------------------------------------------------------------------------
int check_weights(const tt_mpnet_weights* w) {
    TT_CHECK_ARG(w != nullptr, "null weights");
    const tt_encoder_weights& e = w->enc;
    if (int rc = check_postln_shape("mpnet", e.hidden, e.heads, e.ffn, 128)) return rc;
    TT_CHECK_ARG(e.layers >= 0 && (e.layers == 0 || e.layer != nullptr), "layer array missing");
    TT_CHECK_ARG(e.word_emb && e.pos_emb && e.emb_ln_g && e.emb_ln_b && e.vocab > 0 && e.max_pos > 0, "embedding tables missing");
    TT_CHECK_ARG(e.ln_eps > 0.f, "ln_eps=%g", e.ln_eps);
    TT_CHECK_ARG(w->rel_bias && w->bias_table, "rel_bias / bias_table missing");
    for (int l = 0; l < e.layers; ++l) {
        const tt_layer_weights& lw = e.layer[l];
        if (lw.qkv_w8 || lw.qkv_wscale || lw.ffn1_w8 || lw.ffn1_wscale || lw.o_w8 || lw.o_wscale || lw.ffn2_w8 || lw.ffn2_wscale) {
            tt_set_error("mpnet: layer %d carries fp8 projections (qkv_w8 / ffn1_w8 / o_w8 / ffn2_w8): the MPNet path has none", l);
            return TT_E_UNSUPPORTED;
        }
    }
    return TT_OK;
}

// the zeros are the embedding kernel's token-type row
PostLnDims mp_dims(const tt_mpnet_weights* w) {
    const tt_encoder_weights& e = w->enc;
    return {e.hidden, e.heads, e.ffn, e.layers, e.ln_eps, QkvForm::SplitV8, false, (size_t)e.hidden * 2, 0};
}

// what postln.h's driver asks of a family
struct MpFamily {
    const tt_mpnet_weights* w;
    const int32_t *ids, *pos;

    int embed(const float* zero, uint16_t* out, int T, hipStream_t st) const {
        const tt_encoder_weights& ew = w->enc;
        EmbedParams ep{};
        ep.ids = ids; ep.pos = pos; ep.type = nullptr;
        ep.word = (const uint16_t*)ew.word_emb; ep.posemb = (const uint16_t*)ew.pos_emb;
        ep.typeemb = (const uint16_t*)zero;   // no token types: type 0 of a one-row table of zeros
        ep.gamma = ew.emb_ln_g; ep.beta = ew.emb_ln_b;
        ep.T = T; ep.H = ew.hidden; ep.vocab = ew.vocab; ep.max_pos = ew.max_pos; ep.type_vocab = 1;
        ep.eps = ew.ln_eps;
        ep.out = out;
        return tt_embed_ln_launch(ep, st);
    }
    PostLnLayer layer(int l, const float*) const { return postln_layer_of(w->enc.layer[l]); }
    int attention(int, const PostLnBufs& b, const PackedSeqs& s, hipStream_t st) const {
        const int H = w->enc.hidden;
        return relbias_attention_launch(b.qkv, 2 * H, 0, H, b.vt, 8 * H, b.ctx, H, s.seq_start, s.seq_len, s.n_seq, s.n_rows, w->enc.heads,
                                        s.max_len, w->bias_table, st);
    }
};

}  // namespace

extern "C" {

size_t tt_mpnet_workspace_bytes(const tt_mpnet_weights* w, int n_rows) {
    if (!w || n_rows <= 0 || check_weights(w) != TT_OK) return 0;
    return postln_plan(mp_dims(w), n_rows).total;
}

int tt_mpnet_forward(const tt_mpnet_weights* w, const int32_t* ids, const int32_t* pos, const int32_t* type_ids,
                     const int32_t* seq_start, const int32_t* seq_len, int n_seq, int n_rows, int max_len, void* hidden_out,
                     void* workspace, size_t workspace_bytes, void* stream) {
    if (int rc = check_weights(w)) return rc;
    const PostLnDims d = mp_dims(w);
    if (int rc = check_packed_forward_args("tt_mpnet_forward", "MPNet", ids, pos, type_ids, seq_start, seq_len, n_seq, n_rows, max_len,
                                           hidden_out, workspace, workspace_bytes, postln_plan(d, n_rows).total))
        return rc;
    for (int l = 0; l < w->enc.layers; ++l) {
        const tt_layer_weights& lw = w->enc.layer[l];
        TT_CHECK_ARG(lw.qkv_w && lw.qkv_b && lw.o_w && lw.o_b && lw.ln1_g && lw.ln1_b && lw.ffn1_w && lw.ffn1_b && lw.ffn2_w &&
                         lw.ffn2_b && lw.ln2_g && lw.ln2_b,
                     "layer %d has a null weight pointer", l);
    }
    return postln_run<void>(d, MpFamily{w, ids, pos}, PackedSeqs{seq_start, seq_len, n_seq, n_rows, max_len}, hidden_out, workspace,
                            (hipStream_t)stream);
}

int tt_attention_relbias(const void* qkv, int ld, int q_col0, int k_col0, const void* vt, int ldvt, void* out, int ld_out,
                         const int32_t* seq_start, const int32_t* seq_len, int n_seq, int n_rows, int heads, int head_dim,
                         int max_len, const float* bias_table, void* stream) {
    if (int rc = check_attention_layout("relative-position attention", bias_table != nullptr, qkv, ld, q_col0, k_col0, vt, ldvt, out,
                                        ld_out, seq_start, seq_len, n_seq, n_rows, heads, head_dim, max_len))
        return rc;
    return relbias_attention_launch((const uint16_t*)qkv, ld, q_col0, k_col0, (const uint16_t*)vt, ldvt, (uint16_t*)out, ld_out, seq_start,
                                    seq_len, n_seq, n_rows, heads, max_len, bias_table, (hipStream_t)stream);
}

}  // extern "C"
