// DeBERTa-v2 / v3 cross-encoders (DebertaV2ForSequenceClassification: mixedbread-ai/mxbai-rerank-*-v1, the cross-encoder/*-deberta-v3-*
// checkpoints, fine-tunes of microsoft/deberta-v3-*): the whole-model forward, the classification head and the kernels that only
// this family needs (include/tt_hip.h, "DeBERTa-v2 / v3 cross-encoders").  The layer is the post-LN BERT block of encoder_api.hip with
// DISENTANGLED attention: besides the content score Q[q] . K[k], every (query, key) pair gets a content-to-position and a
// position-to-content term that depend on the bucket of its distance,
//   i(q, k) = dist_index[q - k]                         (the host's table over the distance: log buckets, no logarithm here)
//   score   = (Q[q] . K[k] + Q[q] . PK[i] + K[k] . PQ[i]) / sqrt(3 * 64)
// with PK / PQ this layer's key / query projection of the normalised relative embeddings, [n_pos][H], built once per checkpoint by
// the host.  The embedding + LayerNorm, the projections and the LayerNorms are the encoder's own launches (rowops.hip, gemm.hip);
// the attention is the shared one-wave tile (varlen.h attention_tile) with the Disentangled policy.
//
// Layer schedule (one rounding to the element type per fused kernel output):
//   qk, vT = QKV-GEMM(x)                       [T][2H] + the V8 layout [T/8][H][8]
//   C, P   = tables(qk; PK, PQ)                fp32 [T][heads][n_pos] each: C[t][h][w] = Q[t,h] . PK[w,h], P[t][h][w] = K[t,h] . PQ[w,h],
//                                              w over the indices a distance below the batch's longest sequence can reach
//   ctx    = attention(qk, vT; C, P)           [T][H]   softmax((q.k + C[q][i] + P[k][i]) / sqrt(192)), bidirectional
//   y      = GEMM(ctx, Wo) + bo + x            residual fused in the epilogue
//   x1     = LayerNorm(y)
//   f      = GELU(GEMM(x1, W1) + b1)           [T][F]
//   y      = GEMM(f, W2) + b2 + x1
//   x      = LayerNorm(y)
// with x = LayerNorm(word[ids]) before the first layer: no absolute positions (position_biased_input false) and no token types --
// the embedding kernel's position and type rows are one row of zeros in the workspace.
//
// Compiled twice like the encoder path (common.h TT_F16): bf16 and fp16 (external names with an _f16 suffix, f16_names.h).
#include "postln.h"

namespace {

// ---- the two position score tables of one layer ------------------------------------------------------------------------------------
// One workgroup of four waves per (16 rows, head, table): out[t][h][w] = X[t, h] . PW[w, h] in fp32, X the Q (table C) or K (table P)
// columns of the rows, PW pos_key or pos_query.  A wave takes every fourth 16-index tile of [i_lo, i_hi], the indices the distances
// of this batch reach (dist_index is non-decreasing in the distance); one mfma 16x16x32 pair per tile with the indices as rows, so
// a lane ends up with four consecutive indices of one row: a 16-byte store.
__global__ __launch_bounds__(256) void dis_tables_kernel(const uint16_t* __restrict__ qkv, int ld, int q_col0, int k_col0,
                                                         const uint16_t* __restrict__ pos_key, const uint16_t* __restrict__ pos_query,
                                                         int n_pos, const int32_t* __restrict__ dist_index, int max_pos, int max_len,
                                                         int n_rows, int heads, float* __restrict__ c_tab, float* __restrict__ p_tab) {
    const int t0 = blockIdx.x * 16, h = blockIdx.y, which = blockIdx.z;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, c = lane & 15, g = lane >> 4;
    const int reach = min(max_len, max_pos) - 1;
    const int i_lo = min(max(dist_index[max_pos - 1 - reach], 0), n_pos - 1);
    const int i_hi = min(max(dist_index[max_pos - 1 + reach], 0), n_pos - 1);
    const int ldp = heads * 64;
    const uint16_t* x = qkv + (which ? k_col0 : q_col0) + h * 64 + 8 * g;
    const uint16_t* pw = (which ? pos_query : pos_key) + h * 64 + 8 * g;
    float* out = (which ? p_tab : c_tab) + (size_t)h * n_pos;
    const size_t ld_out = (size_t)heads * n_pos;
    const uint4 zero4 = uint4{0u, 0u, 0u, 0u};
    const int row = t0 + c;
    ex8 xf[2];   // the B operand: lane holds X[t0 + c][32 kk + 8 g + j]
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) {
        const uint4 u = row < n_rows ? *reinterpret_cast<const uint4*>(x + (size_t)row * ld + kk * 32) : zero4;
        xf[kk] = __builtin_bit_cast(ex8, u);
    }
    for (int wt = (i_lo >> 4) + wv; 16 * wt <= i_hi; wt += 4) {
        const int wr = 16 * wt + c;   // A row c: index 16 wt + c; result row 4 g + i is index 16 wt + 4 g + i, column c is row t0 + c
        f32x4 acc = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int kk = 0; kk < 2; ++kk) {
            const uint4 u = wr < n_pos ? *reinterpret_cast<const uint4*>(pw + (size_t)wr * ldp + kk * 32) : zero4;
            acc = TT_MFMA_16x16x32(__builtin_bit_cast(ex8, u), xf[kk], acc);
        }
        const int w0 = 16 * wt + 4 * g;   // (n_pos is a multiple of 4: the four indices are inside together)
        if (row < n_rows && w0 < n_pos)
            *reinterpret_cast<float4*>(out + (size_t)row * ld_out + w0) = float4{acc[0], acc[1], acc[2], acc[3]};
    }
}

// ---- bidirectional disentangled attention over packed varlen sequences, head_dim 64 ---------------------------------------------
// One wave per (16-query tile, sequence, head) on varlen.h's tile with the window mask (w >= the longest sequence: every key of the
// sequence) and the Disentangled policy; the index table is staged in LDS once per workgroup, before the walk over the sequences.
__global__ __launch_bounds__(64) void dis_attention_kernel(const uint16_t* __restrict__ qkv, int ld, int q_col0, int k_col0,
                                                           const uint16_t* __restrict__ vt, int ldvt, uint16_t* __restrict__ out,
                                                           int ld_out, const int32_t* __restrict__ seq_start,
                                                           const int32_t* __restrict__ seq_len, int n_seq, int n_rows, int w,
                                                           float scale_log2, const int32_t* __restrict__ dist_index, int max_pos,
                                                           int n_pos, int heads, const float* __restrict__ c_tab,
                                                           const float* __restrict__ p_tab) {
    __shared__ int32_t idx_lds[Disentangled::LDS_INTS];
    const int t = blockIdx.x, h = blockIdx.z;
    disent_stage(dist_index, max_pos, n_pos, idx_lds);
    const Disentangled bias{idx_lds, max_pos - 1, 2 * max_pos - 2, c_tab + (size_t)h * n_pos, p_tab + (size_t)h * n_pos,
                            (size_t)heads * n_pos};
    for (int b = blockIdx.y; b < n_seq; b += gridDim.y)   // (wave-uniform: every lane takes the same sequences)
        attention_tile<64, true, Disentangled>(qkv, ld, q_col0, k_col0, vt, ldvt, out, ld_out, seq_start, seq_len, n_rows, 1, w,
                                               scale_log2, b, h, t, -1, 0, bias);
}

// bytes of ONE score table, [n_rows][heads][n_pos] fp32 rounded up to the workspace's 256-byte grid; false: it does not fit in size_t
bool table_bytes(int n_rows, int heads, int n_pos, size_t* bytes) {
    size_t n = 0;
    if (__builtin_mul_overflow((size_t)n_rows, (size_t)heads, &n) || __builtin_mul_overflow(n, (size_t)n_pos, &n) ||
        __builtin_mul_overflow(n, sizeof(float), &n) || n > SIZE_MAX / 4)
        return false;
    *bytes = tt_align_up(n, 256);
    return true;
}

// the tables, then the attention; c_tab / p_tab hold table_bytes() each
int disentangled_attention_launch(const uint16_t* qkv, int ld, int q_col0, int k_col0, const uint16_t* vt, int ldvt, uint16_t* out,
                                  int ld_out, const int32_t* seq_start, const int32_t* seq_len, int n_seq, int n_rows, int heads,
                                  int max_len, const uint16_t* pos_key, const uint16_t* pos_query, int n_pos, const int32_t* dist_index,
                                  int max_pos, float* c_tab, float* p_tab, hipStream_t st) {
    TtProfScope prof(TT_K_ATTENTION, st);
    hipLaunchKernelGGL(dis_tables_kernel, dim3((n_rows + 15) / 16, heads, 2), dim3(256), 0, st, qkv, ld, q_col0, k_col0, pos_key,
                       pos_query, n_pos, dist_index, max_pos, max_len, n_rows, heads, c_tab, p_tab);
    TT_CHECK_LAUNCH();
    const int n_qt = (max_len + 15) / 16;
    const dim3 grid(n_qt, std::min(n_seq, 65535), heads);   // more sequences: each block row takes every 65535th
    const float scale_log2 = 1.4426950408889634f / 13.856406460551018f;   // log2(e) / sqrt(3 * 64)
    // w = n_rows: |q - k| < n_rows within a batch, so the window mask keeps every key of the sequence
    hipLaunchKernelGGL(dis_attention_kernel, grid, dim3(64), 0, st, qkv, ld, q_col0, k_col0, vt, ldvt, out, ld_out, seq_start, seq_len,
                       n_seq, n_rows, n_rows, scale_log2, dist_index, max_pos, n_pos, heads, c_tab, p_tab);
    TT_CHECK_LAUNCH();
    return TT_OK;
}

// ---- classification head: ContextPooler (dense on the first row -> GELU) -> classifier -> sigmoid, fp32 ----------------------------
// One wave (one block) per sequence, modernbert.hip's head without the pooling choice and the norm.  The first row goes to LDS; lane
// l owns the dense outputs l, l + 64, ... and walks the inputs in ascending order over the TRANSPOSED matrix (coalesced rows), so a
// sequence's logit does not depend on the batch it travels in.
__global__ __launch_bounds__(64) void dis_head_kernel(const uint16_t* __restrict__ hidden, int ld, const int32_t* __restrict__ seq_start,
                                                      int H, const float* __restrict__ dense_wt, const float* __restrict__ dense_b,
                                                      const float* __restrict__ cls_w, const float* __restrict__ cls_b,
                                                      float* __restrict__ scores, float* __restrict__ logits) {
    __shared__ float pooled[1024];
    const int b = blockIdx.x, lane = threadIdx.x;
    const int s0 = seq_start[b];
    for (int i = lane; i < H; i += 64) pooled[i] = s0 >= 0 ? ebits_to_f32(hidden[(size_t)s0 * ld + i]) : 0.f;
    __syncthreads();
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
    float dot = 0.f;
#pragma unroll
    for (int jj = 0; jj < 16; ++jj) {
        if (jj < no) {
            const int o = lane + 64 * jj;
            const float v = y[jj] + dense_b[o];
            dot += 0.5f * v * (1.0f + erff(v * 0.70710678118654752f)) * cls_w[o];   // (libm erf: a few hundred rows per call)
        }
    }
    dot = wave_sum(dot) + cls_b[0];
    if (lane == 0) {
        scores[b] = 1.0f / (1.0f + expf(-dot));
        if (logits) logits[b] = dot;
    }
}

// ---- argument checks -----------------------------------------------------------------------------------------------------------
int check_tables(int n_pos, int max_pos) {
    if (n_pos <= 0 || n_pos % 4) {
        tt_set_error("deberta: n_pos=%d (2 * position_buckets) must be a positive multiple of 4", n_pos);
        return TT_E_UNSUPPORTED;
    }
    if (max_pos <= 0 || max_pos > Disentangled::MAX_POS) {
        tt_set_error("deberta: max_pos=%d must be in 1..%d (the index table a workgroup stages)", max_pos, Disentangled::MAX_POS);
        return TT_E_UNSUPPORTED;
    }
    return TT_OK;
}

int check_weights(const tt_deberta_weights* w) {
    TT_CHECK_ARG(w != nullptr, "null weights");
    const tt_encoder_weights& e = w->enc;
    if (int rc = check_postln_shape("deberta", e.hidden, e.heads, e.ffn, 128)) return rc;
    if (int rc = check_tables(w->n_pos, w->max_pos)) return rc;
    TT_CHECK_ARG(e.layers >= 0 && (e.layers == 0 || e.layer != nullptr), "layer array missing");
    TT_CHECK_ARG(e.word_emb && e.emb_ln_g && e.emb_ln_b && e.vocab > 0, "embedding tables missing");
    TT_CHECK_ARG(e.ln_eps > 0.f, "ln_eps=%g", e.ln_eps);
    TT_CHECK_ARG(w->dist_index && (e.layers == 0 || (w->pos_key && w->pos_query)), "pos_key / pos_query / dist_index missing");
    for (int l = 0; l < e.layers; ++l) {
        const tt_layer_weights& lw = e.layer[l];
        if (lw.qkv_w8 || lw.qkv_wscale || lw.ffn1_w8 || lw.ffn1_wscale || lw.o_w8 || lw.o_wscale || lw.ffn2_w8 || lw.ffn2_wscale) {
            tt_set_error("deberta: layer %d carries fp8 projections (qkv_w8 / ffn1_w8 / o_w8 / ffn2_w8): the DeBERTa path has none", l);
            return TT_E_UNSUPPORTED;
        }
        TT_CHECK_ARG(w->pos_key[l] && w->pos_query[l], "layer %d has no pos_key / pos_query", l);
    }
    return TT_OK;
}

// the forward's shape for postln.h; the zeros are the embedding kernel's position and token-type row, the tail the two score tables
// of *tb bytes each (n_rows * heads * n_pos * 8 bytes together).  false: the tables do not fit in size_t, and the tail is left out
bool db_dims(const tt_deberta_weights* w, int n_rows, PostLnDims* d, size_t* tb) {
    const tt_encoder_weights& e = w->enc;
    *d = {e.hidden, e.heads, e.ffn, e.layers, e.ln_eps, QkvForm::SplitV8, false, (size_t)e.hidden * 2, 0};
    *tb = 0;
    const bool fits = table_bytes(n_rows, e.heads, w->n_pos, tb) && *tb <= (SIZE_MAX - postln_plan(*d, n_rows).total) / 2;
    if (fits && e.layers > 0) d->tail_bytes = 2 * *tb;
    return fits;
}

// what postln.h's driver asks of a family
struct DbFamily {
    const tt_deberta_weights* w;
    const int32_t *ids, *pos;
    size_t tb;   // bytes of one score table in the workspace's tail

    int embed(const float* zero, uint16_t* out, int T, hipStream_t st) const {
        const tt_encoder_weights& ew = w->enc;
        EmbedParams ep{};
        // no absolute positions, no token types: position 0 and type 0 of a one-row table of zeros (max_pos 1 clamps whatever pos holds)
        ep.ids = ids; ep.pos = pos; ep.type = nullptr;
        ep.word = (const uint16_t*)ew.word_emb;
        ep.posemb = (const uint16_t*)zero;
        ep.typeemb = (const uint16_t*)zero;
        ep.gamma = ew.emb_ln_g; ep.beta = ew.emb_ln_b;
        ep.T = T; ep.H = ew.hidden; ep.vocab = ew.vocab; ep.max_pos = 1; ep.type_vocab = 1;
        ep.eps = ew.ln_eps;
        ep.out = out;
        return tt_embed_ln_launch(ep, st);
    }
    PostLnLayer layer(int l, const float*) const { return postln_layer_of(w->enc.layer[l]); }
    int attention(int l, const PostLnBufs& b, const PackedSeqs& s, hipStream_t st) const {
        const int H = w->enc.hidden;
        return disentangled_attention_launch(b.qkv, 2 * H, 0, H, b.vt, 8 * H, b.ctx, H, s.seq_start, s.seq_len, s.n_seq, s.n_rows,
                                             w->enc.heads, s.max_len, (const uint16_t*)w->pos_key[l], (const uint16_t*)w->pos_query[l],
                                             w->n_pos, w->dist_index, w->max_pos, (float*)b.tail, (float*)(b.tail + tb), st);
    }
};

}  // namespace

extern "C" {

size_t tt_deberta_workspace_bytes(const tt_deberta_weights* w, int n_rows) {
    if (!w || n_rows <= 0 || check_weights(w) != TT_OK) return 0;
    PostLnDims d;
    size_t tb;
    return db_dims(w, n_rows, &d, &tb) ? postln_plan(d, n_rows).total : 0;
}

int tt_deberta_forward(const tt_deberta_weights* w, const int32_t* ids, const int32_t* pos, const int32_t* type_ids,
                       const int32_t* seq_start, const int32_t* seq_len, int n_seq, int n_rows, int max_len, void* hidden_out,
                       void* workspace, size_t workspace_bytes, void* stream) {
    if (int rc = check_weights(w)) return rc;
    PostLnDims d;
    size_t tb;
    TT_CHECK_ARG(db_dims(w, n_rows > 0 ? n_rows : 1, &d, &tb), "n_rows=%d heads=%d n_pos=%d: the score tables do not fit in size_t",
                 n_rows, w->enc.heads, w->n_pos);
    if (int rc = check_packed_forward_args("tt_deberta_forward", "DeBERTa", ids, pos, type_ids, seq_start, seq_len, n_seq, n_rows, max_len,
                                           hidden_out, workspace, workspace_bytes, postln_plan(d, n_rows > 0 ? n_rows : 1).total))
        return rc;
    TT_CHECK_ARG(max_len <= w->max_pos, "max_len=%d exceeds max_pos=%d", max_len, w->max_pos);
    for (int l = 0; l < w->enc.layers; ++l) {
        const tt_layer_weights& lw = w->enc.layer[l];
        TT_CHECK_ARG(lw.qkv_w && lw.qkv_b && lw.o_w && lw.o_b && lw.ln1_g && lw.ln1_b && lw.ffn1_w && lw.ffn1_b && lw.ffn2_w &&
                         lw.ffn2_b && lw.ln2_g && lw.ln2_b,
                     "layer %d has a null weight pointer", l);
    }
    return postln_run<void>(d, DbFamily{w, ids, pos, tb}, PackedSeqs{seq_start, seq_len, n_seq, n_rows, max_len}, hidden_out, workspace,
                            (hipStream_t)stream);
}

int tt_deberta_head(const tt_deberta_weights* w, const void* hidden, int ld, const int32_t* seq_start, const int32_t* seq_len,
                    int n_seq, int pooling, float* scores, float* logits, void* stream) {
    (void)seq_len;
    if (int rc = check_weights(w)) return rc;
    TT_CHECK_ARG(n_seq > 0, "n_seq=%d", n_seq);
    TT_CHECK_ARG(pooling == 0, "pooling=%d (ContextPooler reads the first token: 0)", pooling);
    TT_CHECK_ARG(hidden && seq_start && scores, "null pointer");
    TT_CHECK_ARG(w->pooler_dense_wt && w->pooler_dense_b && w->cls_w && w->cls_b, "these weights carry no classification head");
    TT_CHECK_ARG(ld >= w->enc.hidden, "hidden=%d ld=%d", w->enc.hidden, ld);
    hipStream_t st = (hipStream_t)stream;
    TtProfScope prof(TT_K_ROWOPS, st);
    hipLaunchKernelGGL(dis_head_kernel, dim3(n_seq), dim3(64), 0, st, (const uint16_t*)hidden, ld, seq_start, w->enc.hidden,
                       w->pooler_dense_wt, w->pooler_dense_b, w->cls_w, w->cls_b, scores, logits);
    TT_CHECK_LAUNCH();
    return TT_OK;
}

int tt_attention_disentangled(const void* qkv, int ld, int q_col0, int k_col0, const void* vt, int ldvt, void* out, int ld_out,
                              const int32_t* seq_start, const int32_t* seq_len, int n_seq, int n_rows, int heads, int head_dim,
                              int max_len, const void* pos_key, const void* pos_query, int n_pos, const int32_t* dist_index,
                              int max_pos, void* workspace, size_t workspace_bytes, void* stream) {
    if (int rc = check_attention_layout("disentangled attention", pos_key && pos_query && dist_index, qkv, ld, q_col0, k_col0, vt, ldvt,
                                        out, ld_out, seq_start, seq_len, n_seq, n_rows, heads, head_dim, max_len))
        return rc;
    if (int rc = check_tables(n_pos, max_pos)) return rc;
    TT_CHECK_ARG(max_len <= max_pos, "max_len=%d exceeds max_pos=%d", max_len, max_pos);
    TT_CHECK_ARG(((uintptr_t)pos_key % 16) == 0 && ((uintptr_t)pos_query % 16) == 0, "pos_key / pos_query must be 16-byte aligned");
    size_t tb = 0;
    TT_CHECK_ARG(table_bytes(n_rows, heads, n_pos, &tb), "n_rows=%d heads=%d n_pos=%d: the score tables do not fit in size_t", n_rows,
                 heads, n_pos);
    if (int rc = tt_check_workspace("tt_attention_disentangled", workspace, workspace_bytes, 2 * tb)) return rc;
    return disentangled_attention_launch((const uint16_t*)qkv, ld, q_col0, k_col0, (const uint16_t*)vt, ldvt, (uint16_t*)out, ld_out,
                                         seq_start, seq_len, n_seq, n_rows, heads, max_len, (const uint16_t*)pos_key,
                                         (const uint16_t*)pos_query, n_pos, dist_index, max_pos, (float*)workspace,
                                         (float*)((char*)workspace + tb), (hipStream_t)stream);
}

}  // extern "C"
