// MPNet encoders (MPNetModel embedders: all-mpnet-base-v2, multi-qa-mpnet-base-*): the whole-model forward and the one kernel that
// only this family needs (include/tt_hip.h, "MPNet encoders").  MPNet is the post-LN BERT block of encoder_api.hip with a learned
// relative-position bias added to every layer's attention scores, one [32 buckets][heads] table for all layers.  The embedding +
// LayerNorm, the projections and the LayerNorms are the encoder's own launches (rowops.hip, gemm.hip); the attention is the shared
// one-wave tile (varlen.h attention_tile) with the RelBias policy.
//
// Layer schedule (one rounding to the element type per fused kernel output):
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
#include "varlen.h"

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
    if (e.hidden <= 0 || e.hidden % 128 || e.hidden > 1024) {
        tt_set_error("mpnet: hidden=%d must be a multiple of 128 and <= 1024 (the scan's limit)", e.hidden);
        return TT_E_UNSUPPORTED;
    }
    if (e.heads <= 0 || e.hidden != 64 * e.heads) {
        tt_set_error("mpnet: hidden=%d heads=%d: head_dim must be 64", e.hidden, e.heads);
        return TT_E_UNSUPPORTED;
    }
    if (e.ffn <= 0 || e.ffn % 128) {
        tt_set_error("mpnet: ffn=%d must be a multiple of 128", e.ffn);
        return TT_E_UNSUPPORTED;
    }
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

struct MpWs {
    size_t off_xa, off_xb, off_y, off_qk, off_vt, off_ctx, off_ffn, off_zero, zero_bytes, total;
};

MpWs mp_plan(const tt_mpnet_weights* w, int n_rows) {
    MpWs e{};
    // buffers are sized for a multiple of 256 rows: the attention tile reads whole key blocks
    const size_t H = (size_t)w->enc.hidden, F = (size_t)w->enc.ffn, T = ((size_t)n_rows + 255) / 256 * 256;
    WsPlanner ws;
    e.off_xa = ws.take(T * H * 2);
    e.off_xb = ws.take(T * H * 2);
    e.off_y = ws.take(T * H * 2);
    e.off_qk = ws.take(T * 2 * H * 2);
    e.off_vt = ws.take(H * T * 2);
    e.off_ctx = ws.take(T * H * 2);
    e.off_ffn = ws.take(T * F * 2);
    e.zero_bytes = H * 2;            // the embedding kernel's token-type row
    e.off_zero = ws.take(e.zero_bytes);
    e.total = ws.off;
    return e;
}

// one layer on T rows: x -> out (x1 and y are scratch; out may be x)
int mp_layer(const tt_mpnet_weights* w, const tt_layer_weights& lw, int T, const uint16_t* x, uint16_t* qk, uint16_t* vt, uint16_t* ctx,
             uint16_t* y, uint16_t* x1, uint16_t* ffn, uint16_t* out, const int32_t* seq_start, const int32_t* seq_len, int n_seq,
             int max_len, hipStream_t st) {
    const int H = w->enc.hidden, F = w->enc.ffn;
    const float eps = w->enc.ln_eps;
    GemmParams g = gemm_16(x, lw.qkv_w, lw.qkv_b, T, 3 * H, H);
    g.C = qk; g.ldc = 2 * H; g.vt = vt; g.ldvt = 8 * H; g.vt_col0 = 2 * H;
    if (int rc = tt_gemm_launch(g, TT_EPI_QKV, st)) return rc;
    if (int rc = relbias_attention_launch(qk, 2 * H, 0, H, vt, 8 * H, ctx, H, seq_start, seq_len, n_seq, T, w->enc.heads, max_len,
                                          w->bias_table, st))
        return rc;
    GemmParams go = gemm_16(ctx, lw.o_w, lw.o_b, T, H, H);
    go.residual = x; go.ldr = H; go.C = y; go.ldc = H;
    if (int rc = tt_gemm_launch(go, TT_EPI_RESIDUAL, st)) return rc;
    {
        TtProfScope prof(TT_K_ROWOPS, st);
        if (int rc = tt_layernorm_launch(y, x1, lw.ln1_g, lw.ln1_b, T, H, eps, st)) return rc;
    }
    GemmParams g1 = gemm_16(x1, lw.ffn1_w, lw.ffn1_b, T, F, H);
    g1.C = ffn; g1.ldc = F;
    if (int rc = tt_gemm_launch(g1, TT_EPI_GELU, st)) return rc;
    GemmParams g2 = gemm_16(ffn, lw.ffn2_w, lw.ffn2_b, T, H, F);
    g2.residual = x1; g2.ldr = H; g2.C = y; g2.ldc = H;
    if (int rc = tt_gemm_launch(g2, TT_EPI_RESIDUAL, st)) return rc;
    TtProfScope prof(TT_K_ROWOPS, st);
    return tt_layernorm_launch(y, out, lw.ln2_g, lw.ln2_b, T, H, eps, st);
}

int mp_run(const tt_mpnet_weights* w, const int32_t* ids, const int32_t* pos, const int32_t* seq_start, const int32_t* seq_len,
           int n_seq, int n_rows, int max_len, void* hidden_out, void* workspace, hipStream_t st) {
    const MpWs e = mp_plan(w, n_rows);
    char* ws = (char*)workspace;
    const tt_encoder_weights& ew = w->enc;
    const int H = ew.hidden, T = n_rows;
    uint16_t* xa = (uint16_t*)(ws + e.off_xa);
    uint16_t* xb = (uint16_t*)(ws + e.off_xb);
    uint16_t* y = (uint16_t*)(ws + e.off_y);
    uint16_t* qk = (uint16_t*)(ws + e.off_qk);
    uint16_t* vt = (uint16_t*)(ws + e.off_vt);
    uint16_t* ctx = (uint16_t*)(ws + e.off_ctx);
    uint16_t* ffn = (uint16_t*)(ws + e.off_ffn);
    TT_CHECK_HIP(hipMemsetAsync(ws + e.off_zero, 0, e.zero_bytes, st));
    // rows that belong to no sequence are never written by the attention kernel: keep them finite
    TT_CHECK_HIP(hipMemsetAsync(ctx, 0, (size_t)T * H * 2, st));

    EmbedParams ep{};
    ep.ids = ids; ep.pos = pos; ep.type = nullptr;
    ep.word = (const uint16_t*)ew.word_emb; ep.posemb = (const uint16_t*)ew.pos_emb;
    ep.typeemb = (const uint16_t*)(ws + e.off_zero);   // no token types: type 0 of a one-row table of zeros
    ep.gamma = ew.emb_ln_g; ep.beta = ew.emb_ln_b;
    ep.T = T; ep.H = H; ep.vocab = ew.vocab; ep.max_pos = ew.max_pos; ep.type_vocab = 1;
    ep.eps = ew.ln_eps;
    uint16_t* x = ew.layers == 0 ? (uint16_t*)hidden_out : xa;
    ep.out = x;
    {
        TtProfScope prof(TT_K_ROWOPS, st);
        if (int rc = tt_embed_ln_launch(ep, st)) return rc;
    }
    for (int l = 0; l < ew.layers; ++l) {
        // x1 is free again after the FFN-down GEMM has consumed it as residual; the second LayerNorm's output goes back to x (or
        // straight to hidden_out on the last layer)
        uint16_t* dst = (l == ew.layers - 1) ? (uint16_t*)hidden_out : x;
        if (int rc = mp_layer(w, ew.layer[l], T, x, qk, vt, ctx, y, xb, ffn, dst, seq_start, seq_len, n_seq, max_len, st)) return rc;
        x = dst;
    }
    return TT_OK;
}

}  // namespace

extern "C" {

size_t tt_mpnet_workspace_bytes(const tt_mpnet_weights* w, int n_rows) {
    if (!w || n_rows <= 0 || check_weights(w) != TT_OK) return 0;
    return mp_plan(w, n_rows).total;
}

int tt_mpnet_forward(const tt_mpnet_weights* w, const int32_t* ids, const int32_t* pos, const int32_t* type_ids,
                     const int32_t* seq_start, const int32_t* seq_len, int n_seq, int n_rows, int max_len, void* hidden_out,
                     void* workspace, size_t workspace_bytes, void* stream) {
    if (int rc = check_weights(w)) return rc;
    if (int rc = check_packed_forward_args("tt_mpnet_forward", "MPNet", ids, pos, type_ids, seq_start, seq_len, n_seq, n_rows, max_len,
                                           hidden_out, workspace, workspace_bytes, mp_plan(w, n_rows).total))
        return rc;
    for (int l = 0; l < w->enc.layers; ++l) {
        const tt_layer_weights& lw = w->enc.layer[l];
        TT_CHECK_ARG(lw.qkv_w && lw.qkv_b && lw.o_w && lw.o_b && lw.ln1_g && lw.ln1_b && lw.ffn1_w && lw.ffn1_b && lw.ffn2_w &&
                         lw.ffn2_b && lw.ln2_g && lw.ln2_b,
                     "layer %d has a null weight pointer", l);
    }
    return mp_run(w, ids, pos, seq_start, seq_len, n_seq, n_rows, max_len, hidden_out, workspace, (hipStream_t)stream);
}

int tt_attention_relbias(const void* qkv, int ld, int q_col0, int k_col0, const void* vt, int ldvt, void* out, int ld_out,
                         const int32_t* seq_start, const int32_t* seq_len, int n_seq, int n_rows, int heads, int head_dim,
                         int max_len, const float* bias_table, void* stream) {
    if (head_dim != 64) {
        tt_set_error("relative-position attention: head_dim=%d (supported: 64)", head_dim);
        return TT_E_UNSUPPORTED;
    }
    TT_CHECK_ARG(qkv && vt && out && seq_start && seq_len && bias_table, "null pointer");
    TT_CHECK_ARG(heads > 0 && n_seq > 0 && max_len > 0 && n_rows > 0 && n_rows % 8 == 0 && max_len <= n_rows,
                 "heads=%d n_seq=%d n_rows=%d max_len=%d", heads, n_seq, n_rows, max_len);
    TT_CHECK_ARG(ld % 8 == 0 && q_col0 % 8 == 0 && k_col0 % 8 == 0 && q_col0 >= 0 && k_col0 >= 0 && ld_out % 4 == 0 &&
                     ld >= std::max(q_col0, k_col0) + heads * 64 && ld_out >= heads * 64 && ldvt >= 8 * heads * 64 && ldvt % 8 == 0,
                 "ld=%d q_col0=%d k_col0=%d ld_out=%d ldvt=%d", ld, q_col0, k_col0, ld_out, ldvt);
    return relbias_attention_launch((const uint16_t*)qkv, ld, q_col0, k_col0, (const uint16_t*)vt, ldvt, (uint16_t*)out, ld_out, seq_start,
                                    seq_len, n_seq, n_rows, heads, max_len, bias_table, (hipStream_t)stream);
}

}  // extern "C"
