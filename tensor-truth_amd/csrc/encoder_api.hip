// C-ABI entry points of the encoder (see include/tt_hip.h): whole-model forward, pooling,
// rerank head, and the building blocks exported for the parity tests.
//
// Layer schedule (post-LN BERT / XLM-R block; one rounding to bf16 per fused kernel output):
//   qk, vT = QKV-GEMM(x)                       [T][2H] + token-blocked transposed V [T/8][H][8]
//   ctx    = attention(qk, vT)                 [T][H]
//   y      = GEMM(ctx, Wo) + bo + x            residual fused in the epilogue
//   x1     = LayerNorm(y)
//   f      = GELU(GEMM(x1, W1) + b1)           [T][F]
//   y      = GEMM(f, W2) + b2 + x1
//   x      = LayerNorm(y)
#include "common.h"
#include "encoder.h"

namespace {

struct EncWs {
    size_t off_xa, off_xb, off_y, off_qk, off_vt, off_ctx, off_ffn, total;
    // CLS-only tail of the last layer (rows = sequences, padded to 256)
    size_t off_cctx, off_cx, off_cy, off_cx1, off_cffn, off_rows;
    int n_cls_pad;
    // fp8 forward: e4m3 copy of the current LayerNorm output + its per-row scales
    size_t off_q8, off_q8s, off_q8c;
    bool fp8;
};

// every layer carries fp8 projections and the shapes fit the fp8 GEMM tiles
bool fp8_ready(const tt_encoder_weights* w, int n_rows) {
    if constexpr (kF16) return false;      // (the fp16 instantiation has no e4m3 projections)
    if (w->layers <= 0 || w->hidden % 256 || w->ffn % 256 || n_rows % 256) return false;
    for (int l = 0; l < w->layers; ++l) {
        const tt_layer_weights& lw = w->layer[l];
        if (!lw.qkv_w8 || !lw.qkv_wscale || !lw.ffn1_w8 || !lw.ffn1_wscale) return false;
    }
    return true;
}

EncWs enc_plan(const tt_encoder_weights* w, int n_rows, int n_seq = 0) {
    EncWs e{};
    // buffers are sized for a multiple of 256 rows: the attention kernels read whole key tiles
    const size_t H = (size_t)w->hidden, F = (size_t)w->ffn, T = ((size_t)n_rows + 255) / 256 * 256;
    WsPlanner ws;
    e.off_xa = ws.take(T * H * 2);
    e.off_xb = ws.take(T * H * 2);
    e.off_y = ws.take(T * H * 2);
    e.off_qk = ws.take(T * 2 * H * 2);
    e.off_vt = ws.take(H * T * 2);
    e.off_ctx = ws.take(T * H * 2);
    e.off_ffn = ws.take(T * F * 2);
    e.n_cls_pad = pooled_rows_pad(n_seq, tt_gemm_skinny_enabled());
    if (n_seq > 0) {
        const size_t B = (size_t)e.n_cls_pad;
        e.off_cctx = ws.take(B * H * 2);
        e.off_cx = ws.take(B * H * 2);
        e.off_cy = ws.take(B * H * 2);
        e.off_cx1 = ws.take(B * H * 2);
        e.off_cffn = ws.take(B * F * 2);
    }
    e.fp8 = fp8_ready(w, n_rows);
    if (e.fp8) {
        e.off_q8 = ws.take(T * H);
        e.off_q8s = ws.take(T * 4);
        e.off_q8c = ws.take(T * 4);   // constant row scales (the FFN intermediate's static scale)
    }
    e.total = ws.off;
    return e;
}

int check_weights(const tt_encoder_weights* w) {
    TT_CHECK_ARG(w != nullptr, "null weights");
    TT_CHECK_ARG(w->hidden > 0 && w->hidden % 128 == 0 && w->hidden <= 1024, "hidden=%d unsupported", w->hidden);
    TT_CHECK_ARG(w->heads > 0 && w->hidden % w->heads == 0, "heads=%d", w->heads);
    const int dh = w->hidden / w->heads;
    TT_CHECK_ARG(dh == 64 || dh == 32, "head_dim=%d not in {32,64}", dh);
    TT_CHECK_ARG(w->ffn > 0 && w->ffn % 128 == 0, "ffn=%d must be a multiple of 128", w->ffn);
    TT_CHECK_ARG(w->layers >= 0 && (w->layers == 0 || w->layer != nullptr), "layer array missing");
    TT_CHECK_ARG(w->word_emb && w->pos_emb && w->type_emb && w->emb_ln_g && w->emb_ln_b, "embedding tables missing");
    return TT_OK;
}

}  // namespace

extern "C" {

size_t tt_encoder_workspace_bytes(const tt_encoder_weights* w, int n_rows) {
    if (!w || n_rows <= 0) return 0;
    return enc_plan(w, n_rows).total;
}

static int forward_impl(const tt_encoder_weights* w, const int32_t* ids, const int32_t* pos,
                        const int32_t* type_ids, const int32_t* seq_start, const int32_t* seq_len, int n_seq,
                        int n_rows, int max_len, void* hidden_out, void* cls_out, void* workspace,
                        size_t workspace_bytes, void* stream, const int32_t* key_len = nullptr) {
    // key_len (tt_encoder_forward_keylen): every layer's attention is the key-limited kernel of colbert.hip; NULL: today's path
    if (int rc = check_weights(w)) return rc;
    TT_CHECK_ARG(key_len == nullptr || cls_out == nullptr, "key_len: the full forward only");
    TT_CHECK_ARG(n_rows > 0 && (n_rows % 128 == 0 || (n_rows < 256 && n_rows % 64 == 0)),
                 "n_rows=%d must be a positive multiple of 128 (or 64 / 192)", n_rows);
    TT_CHECK_ARG(n_seq > 0 && max_len > 0, "n_seq=%d max_len=%d", n_seq, max_len);
    TT_CHECK_ARG(ids && pos && seq_start && seq_len && (hidden_out || cls_out), "null pointer");
    const bool cls_tail = cls_out != nullptr && w->layers > 0;
    const EncWs e = enc_plan(w, n_rows, cls_tail ? n_seq : 0);
    if (int rc = tt_check_workspace("tt_encoder_forward", workspace, workspace_bytes, e.total)) return rc;
    hipStream_t st = (hipStream_t)stream;
    char* ws = (char*)workspace;
    const int H = w->hidden, F = w->ffn, T = n_rows;
    uint16_t* xa = (uint16_t*)(ws + e.off_xa);
    uint16_t* xb = (uint16_t*)(ws + e.off_xb);
    uint16_t* y = (uint16_t*)(ws + e.off_y);
    uint16_t* qk = (uint16_t*)(ws + e.off_qk);
    uint16_t* vt = (uint16_t*)(ws + e.off_vt);
    uint16_t* ctx = (uint16_t*)(ws + e.off_ctx);
    uint16_t* ffn = (uint16_t*)(ws + e.off_ffn);
    // rows that belong to no sequence are never written by the attention kernel
    TT_CHECK_HIP(hipMemsetAsync(ctx, 0, (size_t)T * H * 2, st));

    EmbedParams ep{};
    ep.ids = ids; ep.pos = pos; ep.type = type_ids;
    ep.word = (const uint16_t*)w->word_emb; ep.posemb = (const uint16_t*)w->pos_emb;
    ep.typeemb = (const uint16_t*)w->type_emb;
    ep.gamma = w->emb_ln_g; ep.beta = w->emb_ln_b;
    ep.T = T; ep.H = H; ep.vocab = w->vocab; ep.max_pos = w->max_pos; ep.type_vocab = w->type_vocab;
    ep.eps = w->ln_eps;
    uint16_t* x = (w->layers == 0 && hidden_out) ? (uint16_t*)hidden_out : xa;
    ep.out = x;
    uint8_t* q8 = e.fp8 ? (uint8_t*)(ws + e.off_q8) : nullptr;
    float* q8s = e.fp8 ? (float*)(ws + e.off_q8s) : nullptr;
    ep.q8 = q8; ep.q8_scale = q8s;
    {
        TtProfScope prof(TT_K_ROWOPS, st);
        if (int rc = tt_embed_ln_launch(ep, st)) return rc;
    }

    const int dh = H / w->heads;
    // TT_FP8_MASK (DIAGNOSTIC LIBRARY ONLY, `make DIAG=1`; default 0xF; read per forward there so that one process can sweep it): which projections of an fp8
    // forward run in e4m3 -- bit 0 QKV, 1 attention output, 2 FFN-up, 3 FFN-down (needs bit 2: the intermediate is then
    // written as e4m3); the others stay bf16.  TT_FP8_SKIP_FIRST / TT_FP8_SKIP_LAST: that many layers at either end stay bf16
    // altogether (tools/probes/fp8_sensitivity.py: rank agreement with the fp32 path per setting).
    const int f8mask_all = TT_DIAG_ENV_INT("TT_FP8_MASK", 0xF), f8first = TT_DIAG_ENV_INT("TT_FP8_SKIP_FIRST", 0),
              f8last = TT_DIAG_ENV_INT("TT_FP8_SKIP_LAST", 0);
    // The post-attention half of a layer on M rows: y = GEMM(c, Wo) + bo + res, x1 = LayerNorm(y), f = GELU(GEMM(x1, W1) + b1),
    // y = GEMM(f, W2) + b2 + x1, out = LayerNorm(y).  `f8` names what an fp8 forward adds on its full pass; the CLS tail passes
    // Fp8Ops{}: plain 16-bit weights, no e4m3 copies, no calibration hook.
    struct Fp8Ops {
        uint8_t* q8;      // e4m3 copy of the current GEMM A operand (written by the LayerNorms and by tt_quantize_rows_launch)
        float* q8s;       // its per-row scales
        float* q8c;       // constant row scales of the e4m3 FFN intermediate
        int mask;         // which projections run in e4m3 (TT_FP8_MASK bits; 0 = none)
        float* absmax;    // the layer's entry of ffn_absmax_out, or NULL
    };
    auto half_layer = [&](const tt_layer_weights& lw, int M, uint16_t* c, const uint16_t* res, uint16_t* y, uint16_t* x1, uint16_t* f,
                          uint16_t* out, const Fp8Ops& f8) -> int {
        // attention output projection + residual, LayerNorm
        GemmParams go = gemm_16(c, lw.o_w, lw.o_b, M, H, H);
        go.residual = res; go.ldr = H; go.C = y; go.ldc = H;
        if ((f8.mask & 2) && lw.o_w8 && lw.o_wscale) {   // the QKV GEMM is done with q8: reuse it for the context's e4m3 copy
            {
                TtProfScope prof(TT_K_ROWOPS, st);
                if (int rc = tt_quantize_rows_launch(c, H, M, H, f8.q8, f8.q8s, st)) return rc;
            }
            go.A = (const uint16_t*)f8.q8; go.W = (const uint16_t*)lw.o_w8; go.a_scale = f8.q8s; go.w_scale = lw.o_wscale; go.fp8 = 1;
        }
        if (int rc = tt_gemm_launch(go, TT_EPI_RESIDUAL, st)) return rc;
        {
            TtProfScope prof(TT_K_ROWOPS, st);
            if (int rc = tt_layernorm_launch(y, x1, lw.ln1_g, lw.ln1_b, M, H, w->ln_eps, st, f8.q8, f8.q8s)) return rc;
        }
        // FFN
        GemmParams g1 = gemm_16(x1, lw.ffn1_w, lw.ffn1_b, M, F, H);
        g1.C = f; g1.ldc = F;
        const bool f8down = (f8.mask & 12) == 12 && lw.ffn2_w8 && lw.ffn2_wscale && lw.ffn_act_scale > 0.f;
        if (f8.mask & 4) {
            g1.A = (const uint16_t*)f8.q8; g1.W = (const uint16_t*)lw.ffn1_w8; g1.a_scale = f8.q8s; g1.w_scale = lw.ffn1_wscale; g1.fp8 = 1;
            if (f8down) {   // the intermediate is written as e4m3 (static scale) into the same buffer, half its size
                g1.C8 = (uint8_t*)f; g1.c8_inv_scale = 1.0f / lw.ffn_act_scale;
            }
        }
        if (int rc = tt_gemm_launch(g1, TT_EPI_GELU, st)) return rc;
        if (f8.absmax && !f8down) {
            TtProfScope prof(TT_K_ROWOPS, st);
            if (int rc = tt_absmax_launch(f, (size_t)M * F, f8.absmax, st)) return rc;
        }
        GemmParams g2 = gemm_16(f, lw.ffn2_w, lw.ffn2_b, M, H, F);
        g2.residual = x1; g2.ldr = H; g2.C = y; g2.ldc = H;
        if (f8down) {
            const unsigned bits = __builtin_bit_cast(unsigned, lw.ffn_act_scale);
            TT_CHECK_HIP(hipMemsetD32Async(f8.q8c, (int)bits, (size_t)M, st));
            g2.W = (const uint16_t*)lw.ffn2_w8; g2.a_scale = f8.q8c; g2.w_scale = lw.ffn2_wscale; g2.fp8 = 1;
        }
        if (int rc = tt_gemm_launch(g2, TT_EPI_RESIDUAL, st)) return rc;
        TtProfScope prof(TT_K_ROWOPS, st);
        return tt_layernorm_launch(y, out, lw.ln2_g, lw.ln2_b, M, H, w->ln_eps, st, f8.q8, f8.q8s);
    };
    for (int l = 0; l < w->layers; ++l) {
        const tt_layer_weights& lw = w->layer[l];
        TT_CHECK_ARG(lw.qkv_w && lw.qkv_b && lw.o_w && lw.o_b && lw.ln1_g && lw.ln1_b && lw.ffn1_w && lw.ffn1_b &&
                         lw.ffn2_w && lw.ffn2_b && lw.ln2_g && lw.ln2_b,
                     "layer %d has a null weight pointer", l);
        // QKV projection
        GemmParams g = gemm_16(x, lw.qkv_w, lw.qkv_b, T, 3 * H, H);
        g.C = qk; g.ldc = 2 * H; g.vt = vt; g.ldvt = 8 * H; g.vt_col0 = 2 * H;
        const int f8mask = (!e.fp8 || l < f8first || l >= w->layers - f8last) ? 0 : f8mask_all;
        if (f8mask & 1) {   // x's e4m3 copy and row scales come from the LayerNorm that produced x
            g.A = (const uint16_t*)q8; g.W = (const uint16_t*)lw.qkv_w8; g.a_scale = q8s; g.w_scale = lw.qkv_wscale; g.fp8 = 1;
        }
        // last layer of the CLS tail: only the first row of every sequence needs a QUERY, so the big projection computes K and V alone
        // (the weight rows H..3H; K lands in its usual columns H..2H of qk) and the queries come from a small GEMM over the gathered
        // first rows below.  Same kernels, same K order per output element: bit-identical to the full projection.  Not for the e4m3
        // projection (byte-sized weights); TT_CLS_KV_ONLY=0 restores the full projection (A/B; both sides give the same bits,
        // tests/test_encoder_gpu.py compares them from two processes: the switch is read ONCE).
        static const bool kv_only_on = TT_DIAG_ENV_INT("TT_CLS_KV_ONLY", 1) != 0;
        const bool kv_only = cls_tail && l == w->layers - 1 && !g.fp8 && kv_only_on;
        if (kv_only) {
            g.W = (const uint16_t*)lw.qkv_w + (size_t)H * H; g.bias = lw.qkv_b + H;
            g.C = qk + H; g.N = 2 * H; g.vt_col0 = H;
        }
        if (int rc = tt_gemm_launch(g, TT_EPI_QKV, st)) return rc;
        AttnParams a{};
        a.qk = qk; a.ld_qk = 2 * H; a.q_col0 = 0; a.k_col0 = H; a.vt = vt; a.ldvt = 8 * H;
        a.ld_out = H; a.seq_start = seq_start; a.seq_len = seq_len;
        a.n_seq = n_seq; a.heads = w->heads; a.head_dim = dh; a.max_len = max_len;
        a.scale = 1.0f / sqrtf((float)dh);
        if (cls_tail && l == w->layers - 1) {
            // ---- last layer, CLS rows only: attention of the one query row per sequence, then the
            //      second half of the layer on n_seq (padded) rows instead of n_rows
            const int Bp = e.n_cls_pad;
            uint16_t* cctx = (uint16_t*)(ws + e.off_cctx);
            uint16_t* cx = (uint16_t*)(ws + e.off_cx);
            uint16_t* cy = (uint16_t*)(ws + e.off_cy);
            uint16_t* cx1 = (uint16_t*)(ws + e.off_cx1);
            uint16_t* cffn = (uint16_t*)(ws + e.off_cffn);
            TT_CHECK_HIP(hipMemsetAsync(cctx, 0, (size_t)Bp * H * 2, st));
            {
                TtProfScope prof(TT_K_ROWOPS, st);
                if (int rc = tt_gather_rows_launch(x, H, seq_start, n_seq, Bp, H, cx, st)) return rc;
            }
            if (kv_only) {   // the first rows' queries (cy is free until the output projection writes it)
                GemmParams gq = gemm_16(cx, lw.qkv_w, lw.qkv_b, Bp, H, H);
                gq.C = cy; gq.ldc = H;
                if (int rc = tt_gemm_launch(gq, TT_EPI_BIAS, st)) return rc;
                a.q_rows = cy; a.ld_q_rows = H;
            }
            a.out = cctx;
            if (int rc = tt_attention_cls_launch(a, st)) return rc;
            return half_layer(lw, Bp, cctx, cx, cy, cx1, cffn, (uint16_t*)cls_out, Fp8Ops{});
        }
        // attention
        a.out = ctx; a.total_rows = n_rows;
        if (int rc = key_len ? tt_attention_keylimit_launch(a, key_len, st) : tt_attention_launch(a, st)) return rc;
        // x1 is free again after the FFN-down GEMM has consumed it as residual; the second LayerNorm's output
        // goes to the other hidden buffer (or straight to hidden_out on the last layer)
        uint16_t* x1 = (x == xa) ? xb : xa;
        uint16_t* dst = (l == w->layers - 1) ? (uint16_t*)hidden_out : x;
        const Fp8Ops f8{q8, q8s, e.fp8 ? (float*)(ws + e.off_q8c) : nullptr, f8mask, w->ffn_absmax_out ? w->ffn_absmax_out + l : nullptr};
        if (int rc = half_layer(lw, T, ctx, x, y, x1, ffn, dst, f8)) return rc;
        x = dst;
    }
    return TT_OK;
}

int tt_encoder_forward(const tt_encoder_weights* w, const int32_t* ids, const int32_t* pos,
                       const int32_t* type_ids, const int32_t* seq_start, const int32_t* seq_len, int n_seq,
                       int n_rows, int max_len, void* hidden_out, void* workspace, size_t workspace_bytes,
                       void* stream) {
    TT_CHECK_ARG(hidden_out != nullptr, "null hidden_out");
    return forward_impl(w, ids, pos, type_ids, seq_start, seq_len, n_seq, n_rows, max_len, hidden_out, nullptr, workspace,
                        workspace_bytes, stream);
}

int tt_encoder_forward_keylen(const tt_encoder_weights* w, const int32_t* ids, const int32_t* pos, const int32_t* type_ids,
                              const int32_t* seq_start, const int32_t* seq_len, const int32_t* key_len, int n_seq, int n_rows,
                              int max_len, void* hidden_out, void* workspace, size_t workspace_bytes, void* stream) {
    TT_CHECK_ARG(hidden_out != nullptr, "null hidden_out");
    TT_CHECK_ARG(key_len != nullptr, "null key_len");
    return forward_impl(w, ids, pos, type_ids, seq_start, seq_len, n_seq, n_rows, max_len, hidden_out, nullptr, workspace,
                        workspace_bytes, stream, key_len);
}

size_t tt_encoder_cls_workspace_bytes(const tt_encoder_weights* w, int n_rows, int n_seq) {
    if (!w || n_rows <= 0 || n_seq <= 0) return 0;
    return enc_plan(w, n_rows, n_seq).total;
}

int tt_encoder_forward_cls(const tt_encoder_weights* w, const int32_t* ids, const int32_t* pos,
                           const int32_t* type_ids, const int32_t* seq_start, const int32_t* seq_len, int n_seq,
                           int n_rows, int max_len, void* cls_out, void* workspace, size_t workspace_bytes,
                           void* stream) {
    TT_CHECK_ARG(cls_out != nullptr, "null cls_out");
    TT_CHECK_ARG(w && w->layers > 0, "tt_encoder_forward_cls needs at least one layer");
    return forward_impl(w, ids, pos, type_ids, seq_start, seq_len, n_seq, n_rows, max_len, nullptr, cls_out, workspace,
                        workspace_bytes, stream);
}

int tt_embed_pool(const void* hidden_bf16, int ld, const int32_t* rows, int n_seq, int hidden, float* out_f32,
                  void* out_bf16, void* stream) {
    TT_CHECK_ARG(n_seq >= 0, "n_seq=%d", n_seq);
    if (n_seq == 0) return TT_OK;
    TT_CHECK_ARG(hidden_bf16 && rows && out_f32 && ld >= hidden && ld % 8 == 0, "bad argument");
    TtProfScope prof(TT_K_ROWOPS, (hipStream_t)stream);
    return tt_cls_pool_l2norm_launch((const uint16_t*)hidden_bf16, ld, rows, n_seq, hidden, out_f32,
                                     (uint16_t*)out_bf16, (hipStream_t)stream);
}

int tt_embed_pool_mean(const void* hidden_bf16, int ld, const int32_t* seq_start, const int32_t* seq_len, int n_seq, int hidden,
                       float* out_f32, void* out_bf16, void* stream) {
    TT_CHECK_ARG(n_seq >= 0, "n_seq=%d", n_seq);
    if (n_seq == 0) return TT_OK;
    TT_CHECK_ARG(hidden_bf16 && seq_start && seq_len && out_f32 && ld >= hidden && ld % 8 == 0, "bad argument");
    TtProfScope prof(TT_K_ROWOPS, (hipStream_t)stream);
    return tt_mean_pool_l2norm_launch(hidden_bf16, 0, ld, seq_start, seq_len, n_seq, hidden, out_f32, (uint16_t*)out_bf16,
                                      (hipStream_t)stream);
}

#if !TT_F16   // bf16 instantiation only
int tt_embed_pool_mean_f32(const float* hidden_f32, int ld, const int32_t* seq_start, const int32_t* seq_len, int n_seq, int hidden,
                           float* out_f32, void* out_bf16, void* stream) {
    TT_CHECK_ARG(n_seq >= 0, "n_seq=%d", n_seq);
    if (n_seq == 0) return TT_OK;
    TT_CHECK_ARG(hidden_f32 && seq_start && seq_len && out_f32 && ld >= hidden && ld % 4 == 0, "bad argument");
    TtProfScope prof(TT_K_ROWOPS, (hipStream_t)stream);
    return tt_mean_pool_l2norm_launch(hidden_f32, 1, ld, seq_start, seq_len, n_seq, hidden, out_f32, (uint16_t*)out_bf16,
                                      (hipStream_t)stream);
}

#endif
int tt_rerank_head(const tt_encoder_weights* w, const void* hidden_bf16, const int32_t* rows, int n_seq,
                   float* scores, float* logits, void* workspace, size_t workspace_bytes, void* stream) {
    if (int rc = check_weights(w)) return rc;
    TT_CHECK_ARG(w->cls_dense_w && w->cls_dense_b && w->cls_out_w && w->cls_out_b, "weights carry no classification head");
    TT_CHECK_ARG(n_seq >= 0, "n_seq=%d", n_seq);
    if (n_seq == 0) return TT_OK;
    TT_CHECK_ARG(hidden_bf16 && rows && scores, "null pointer");
    const int H = w->hidden;
    const int n_pad = (n_seq + 127) / 128 * 128;
    const size_t need = 2 * tt_align_up((size_t)n_pad * H * 2, 256);
    if (!workspace || workspace_bytes < need) {
        tt_set_error("tt_rerank_head: workspace %zu < required %zu bytes", workspace_bytes, need);
        return TT_E_WORKSPACE;
    }
    hipStream_t st = (hipStream_t)stream;
    uint16_t* cls = (uint16_t*)workspace;
    uint16_t* t = (uint16_t*)((char*)workspace + tt_align_up((size_t)n_pad * H * 2, 256));
    {
        TtProfScope prof(TT_K_ROWOPS, st);
        if (int rc = tt_gather_rows_launch((const uint16_t*)hidden_bf16, H, rows, n_seq, n_pad, H, cls, st)) return rc;
    }
    GemmParams g{};
    g.A = cls; g.lda = H; g.W = (const uint16_t*)w->cls_dense_w; g.bias = w->cls_dense_b;
    g.C = t; g.ldc = H; g.M = n_pad; g.N = H; g.K = H;
    if (int rc = tt_gemm_launch(g, TT_EPI_TANH, st)) return rc;
    TtProfScope prof(TT_K_ROWOPS, st);
    return tt_head_out_sigmoid_launch(t, H, (const uint16_t*)w->cls_out_w, w->cls_out_b, n_seq, H, scores, logits, st);
}

#if !TT_F16   // bf16 instantiation only
int tt_adjacent_cosine(const float* emb_f32, int n, int hidden, float* out_dist, void* stream) {
    TT_CHECK_ARG(n >= 0, "n=%d", n);
    if (n <= 1) return TT_OK;
    TT_CHECK_ARG(emb_f32 && out_dist, "null pointer");
    TtProfScope prof(TT_K_ROWOPS, (hipStream_t)stream);
    return tt_adjacent_cosine_launch(emb_f32, n, hidden, out_dist, (hipStream_t)stream);
}

#endif
int tt_gemm_bf16(const void* a, const void* w, const float* bias, const void* residual, void* c, int m, int n,
                 int k, int epilogue, void* stream) {
    TT_CHECK_ARG((epilogue >= TT_EPI_BIAS && epilogue <= TT_EPI_TANH) || epilogue == TT_EPI_RELU, "epilogue %d", epilogue);
    GemmParams g{};
    g.A = (const uint16_t*)a; g.lda = k; g.W = (const uint16_t*)w; g.bias = bias;
    g.residual = (const uint16_t*)residual; g.ldr = n; g.C = (uint16_t*)c; g.ldc = n;
    g.M = m; g.N = n; g.K = k;
    return tt_gemm_launch(g, epilogue, (hipStream_t)stream);
}

#if !TT_F16   // bf16 instantiation only
int tt_quantize_rows_fp8(const void* in_bf16, int rows, int cols, void* out_fp8, float* out_scale, void* stream) {
    TT_CHECK_ARG(in_bf16 && out_fp8 && out_scale, "null pointer");
    return tt_quantize_rows_launch((const uint16_t*)in_bf16, cols, rows, cols, (uint8_t*)out_fp8, out_scale, (hipStream_t)stream);
}

int tt_layernorm_bf16_fp8(const void* in, void* out, const float* gamma, const float* beta, int rows, int hidden,
                          float eps, void* out_fp8, float* out_scale, void* stream) {
    TT_CHECK_ARG(in && out && gamma && beta && out_fp8 && out_scale, "null pointer");
    return tt_layernorm_launch((const uint16_t*)in, (uint16_t*)out, gamma, beta, rows, hidden, eps, (hipStream_t)stream,
                               (uint8_t*)out_fp8, out_scale);
}

int tt_gemm_fp8(const void* a8, const float* a_scale, const void* w8, const float* w_scale, const float* bias, void* c,
                int m, int n, int k, int epilogue, void* stream) {
    TT_CHECK_ARG(epilogue == TT_EPI_BIAS || epilogue == TT_EPI_GELU, "epilogue %d", epilogue);
    TT_CHECK_ARG(a8 && a_scale && w8 && w_scale && bias && c, "null pointer");
    GemmParams g{};
    g.A = (const uint16_t*)a8; g.lda = k; g.W = (const uint16_t*)w8; g.bias = bias; g.C = (uint16_t*)c; g.ldc = n;
    g.M = m; g.N = n; g.K = k; g.a_scale = a_scale; g.w_scale = w_scale; g.fp8 = 1;
    return tt_gemm_launch(g, epilogue, (hipStream_t)stream);
}

int tt_gemm_fp8_ex(const void* a8, const float* a_scale, const void* w8, const float* w_scale, const float* bias,
                   const void* residual, void* c_bf16, void* c_fp8, float c_fp8_inv_scale, int m, int n, int k,
                   int epilogue, void* stream) {
    TT_CHECK_ARG(epilogue == TT_EPI_BIAS || epilogue == TT_EPI_GELU || epilogue == TT_EPI_RESIDUAL, "epilogue %d", epilogue);
    TT_CHECK_ARG(a8 && a_scale && w8 && w_scale && bias && (c_bf16 || c_fp8), "null pointer");
    TT_CHECK_ARG(epilogue != TT_EPI_RESIDUAL || (residual && c_bf16 && !c_fp8), "residual epilogue: bf16 result only");
    GemmParams g{};
    g.A = (const uint16_t*)a8; g.lda = k; g.W = (const uint16_t*)w8; g.bias = bias; g.ldc = n;
    // (C only has to be non-null for the launcher's argument check when the result goes to c_fp8)
    g.C = c_bf16 ? (uint16_t*)c_bf16 : (uint16_t*)c_fp8;
    g.residual = (const uint16_t*)residual; g.ldr = n;
    g.M = m; g.N = n; g.K = k; g.a_scale = a_scale; g.w_scale = w_scale; g.fp8 = 1;
    if (c_fp8) { g.C8 = (uint8_t*)c_fp8; g.c8_inv_scale = c_fp8_inv_scale; }
    return tt_gemm_launch(g, epilogue, (hipStream_t)stream);
}

#endif
int tt_layernorm_bf16(const void* in, void* out, const float* gamma, const float* beta, int rows, int hidden,
                      float eps, void* stream) {
    TT_CHECK_ARG(in && out && gamma && beta, "null pointer");
    return tt_layernorm_launch((const uint16_t*)in, (uint16_t*)out, gamma, beta, rows, hidden, eps, (hipStream_t)stream);
}

int tt_attention_varlen(const void* qk, int ld_qk, int q_col0, int k_col0, const void* vt, int ldvt, void* out,
                        int ld_out, const int32_t* seq_start, const int32_t* seq_len, int n_seq, int heads,
                        int head_dim, int max_len, void* stream) {
    TT_CHECK_ARG(qk && vt && out && seq_start && seq_len, "null pointer");
    AttnParams a{};
    a.qk = (const uint16_t*)qk; a.ld_qk = ld_qk; a.q_col0 = q_col0; a.k_col0 = k_col0;
    a.vt = (const uint16_t*)vt; a.ldvt = ldvt; a.out = (uint16_t*)out; a.ld_out = ld_out;
    a.seq_start = seq_start; a.seq_len = seq_len; a.n_seq = n_seq; a.heads = heads; a.head_dim = head_dim;
    a.max_len = max_len; a.scale = 1.0f / sqrtf((float)head_dim);
    return tt_attention_launch(a, (hipStream_t)stream);
}

// the CLS-only kernel of the last layer on tt_attention_varlen's operands: out row b = sequence b's first query row
int tt_attention_cls_varlen(const void* qk, int ld_qk, int q_col0, int k_col0, const void* vt, int ldvt, void* out,
                            int ld_out, const int32_t* seq_start, const int32_t* seq_len, int n_seq, int heads,
                            int head_dim, int max_len, void* stream) {
    TT_CHECK_ARG(qk && vt && out && seq_start && seq_len, "null pointer");
    TT_CHECK_ARG(head_dim == 64 || head_dim == 32, "head_dim=%d: the attention takes 64- or 32-wide heads", head_dim);
    AttnParams a{};
    a.qk = (const uint16_t*)qk; a.ld_qk = ld_qk; a.q_col0 = q_col0; a.k_col0 = k_col0;
    a.vt = (const uint16_t*)vt; a.ldvt = ldvt; a.out = (uint16_t*)out; a.ld_out = ld_out;
    a.seq_start = seq_start; a.seq_len = seq_len; a.n_seq = n_seq; a.heads = heads; a.head_dim = head_dim;
    a.max_len = max_len; a.scale = 1.0f / sqrtf((float)head_dim);
    return tt_attention_cls_launch(a, (hipStream_t)stream);
}

}  // extern "C"
