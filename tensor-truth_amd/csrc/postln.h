// The post-LN BERT block of the packed-varlen families, host side, written once (mpnet.hip: MPNet; deberta.hip: DeBERTa-v2/v3;
// jinabert.hip: JinaBERT; ropebert.hip: NomicBERT / Jina-v3): the shape checks, the workspace plan, the forward's prologue and the
// layer.  No device code here; the kernels are the encoder's (gemm.hip, rowops.hip, attention.hip) and varlen.h's.
//
// Layer schedule (one rounding to the element type per kernel output):
//   QkvForm::SplitV8:  qk, vT = QKV-GEMM(x) + b_qkv     [T][2H] + the V8 layout [T/8][H][8]      (TT_EPI_QKV)
//   QkvForm::Packed:   qkv    = GEMM(x, Wqkv) + b_qkv   [T][3H]; the family's attention fills vT  (TT_EPI_BIAS)
//   ctx = the family's attention(qkv, vT)               [T][H]
//   y   = GEMM(ctx, Wo) + b_o + x                       residual fused in the epilogue            (TT_EPI_RESIDUAL)
//   x1  = LayerNorm(y; ln1)
//   GateAct void:      a  = GELU_erf(GEMM(x1, Wup) + b_up)                      [T][F]            (TT_EPI_GELU)
//   GateAct an Act:    gu = GEMM(x1, Wup) + b_up                                [T][2F]           (TT_EPI_BIAS)
//                      a  = Act::f(gu[:, :F]) * gu[:, F:]                       [T][F]            (varlen.h gated_act_kernel<Act>)
//   y   = GEMM(a, Wdown) + b_down + x1                                                            (TT_EPI_RESIDUAL)
//   x   = LayerNorm(y; ln2)
// with x = the family's embedding launch before the first layer and no norm behind the last.
//
// A family is a small struct the driver is a template over -- no allocation, no indirect call per launch:
//   int embed(const float* zero, uint16_t* out, int T, hipStream_t st) const;         the embedding + LayerNorm launch
//   PostLnLayer layer(int l, const float* zero) const;                                layer l's operands; `zero` for a missing bias
//   int attention(int l, const PostLnBufs& b, const PackedSeqs& s, hipStream_t st) const;   b.qkv (+ b.vt) -> b.ctx
#pragma once
#include "varlen.h"

#include <type_traits>

namespace {

// one layer's operands, whatever the family calls them (tt_layer_weights, tt_jinabert_layer_weights, tt_ropebert_layer_weights)
struct PostLnLayer {
    const void* qkv_w;   // [3H][H]
    const float* qkv_b;
    const void* o_w;     // [H][H]
    const float* o_b;
    const float *ln1_g, *ln1_b;
    const void* up_w;    // [F][H], or gated: [2F][H], the activated rows first
    const float* up_b;
    const void* down_w;  // [H][F]
    const float* down_b;
    const float *ln2_g, *ln2_b;
};

inline PostLnLayer postln_layer_of(const tt_layer_weights& lw) {
    return {lw.qkv_w, lw.qkv_b, lw.o_w, lw.o_b, lw.ln1_g, lw.ln1_b, lw.ffn1_w, lw.ffn1_b, lw.ffn2_w, lw.ffn2_b, lw.ln2_g, lw.ln2_b};
}

struct PostLnDims {
    int hidden, heads, ffn, layers;
    float ln_eps;
    QkvForm qkv;
    bool gated;          // the up-projection is [T][2F] and an activation kernel follows: postln_run's GateAct is not void
    size_t zero_bytes;   // zeros behind the buffers: a missing bias (fp32) or a missing embedding row (element type)
    size_t tail_bytes;   // the family's own scratch behind the zeros (DeBERTa's score tables)
};

// the limits every post-LN family shares: the row ops hold a row of up to 1024 values, the attention kernels take heads of 64, the
// GEMM tiles are 128 columns wide (`ffn_multiple`: 64 where the up-projection is 2F wide)
inline int check_postln_shape(const char* family, int hidden, int heads, int ffn, int ffn_multiple) {
    if (int rc = check_hidden(family, hidden)) return rc;
    if (heads <= 0 || hidden != 64 * heads) {
        tt_set_error("%s: hidden=%d heads=%d: head_dim must be 64", family, hidden, heads);
        return TT_E_UNSUPPORTED;
    }
    if (ffn <= 0 || ffn % ffn_multiple) {
        tt_set_error("%s: ffn=%d must be a multiple of %d", family, ffn, ffn_multiple);
        return TT_E_UNSUPPORTED;
    }
    return TT_OK;
}

// One forward's workspace.  Buffers are sized for a multiple of 256 rows: the attention kernels read whole key blocks.
struct PostLnWs {
    size_t off_x, off_y, off_x1, off_qkv, off_vt, off_ctx, off_gu, off_act, off_zero, off_tail, total;
};

inline PostLnWs postln_plan(const PostLnDims& d, int n_rows) {
    PostLnWs e{};
    const size_t H = (size_t)d.hidden, F = (size_t)d.ffn, T = ((size_t)n_rows + 255) / 256 * 256;
    WsPlanner ws;
    e.off_x = ws.take(T * H * 2);
    e.off_y = ws.take(T * H * 2);
    e.off_x1 = ws.take(T * H * 2);
    e.off_qkv = ws.take(T * (d.qkv == QkvForm::Packed ? 3 : 2) * H * 2);
    e.off_vt = ws.take(T * H * 2);
    e.off_ctx = ws.take(T * H * 2);
    e.off_gu = ws.take(d.gated ? T * 2 * F * 2 : 0);
    e.off_act = ws.take(T * F * 2);
    e.off_zero = ws.take(d.zero_bytes);
    e.off_tail = ws.take(d.tail_bytes);
    e.total = ws.off;
    return e;
}

// the carved workspace
struct PostLnBufs {
    uint16_t *x, *y, *x1, *qkv, *vt, *ctx, *gu, *act;
    const float* zero;
    char* tail;
};

inline int postln_layernorm(const uint16_t* in, uint16_t* out, const float* g, const float* b, int rows, int H, float eps, hipStream_t st) {
    TtProfScope prof(TT_K_ROWOPS, st);
    return tt_layernorm_launch(in, out, g, b, rows, H, eps, st);
}

// one layer on the batch's rows: x -> out (b.x1 and b.y are scratch; out may be x)
template <class GateAct, class Family>
int postln_layer(const PostLnDims& d, const Family& fam, int l, const PostLnBufs& b, const PackedSeqs& s, const uint16_t* x, uint16_t* out,
                 hipStream_t st) {
    const int H = d.hidden, F = d.ffn, T = s.n_rows;
    const PostLnLayer lw = fam.layer(l, b.zero);
    GemmParams g = gemm_16(x, lw.qkv_w, lw.qkv_b, T, 3 * H, H);
    g.C = b.qkv;
    if (d.qkv == QkvForm::SplitV8) {
        g.ldc = 2 * H; g.vt = b.vt; g.ldvt = 8 * H; g.vt_col0 = 2 * H;
        if (int rc = tt_gemm_launch(g, TT_EPI_QKV, st)) return rc;
    } else {
        g.ldc = 3 * H;
        if (int rc = tt_gemm_launch(g, TT_EPI_BIAS, st)) return rc;
    }
    if (int rc = fam.attention(l, b, s, st)) return rc;
    GemmParams go = gemm_16(b.ctx, lw.o_w, lw.o_b, T, H, H);
    go.residual = x; go.ldr = H; go.C = b.y; go.ldc = H;
    if (int rc = tt_gemm_launch(go, TT_EPI_RESIDUAL, st)) return rc;
    if (int rc = postln_layernorm(b.y, b.x1, lw.ln1_g, lw.ln1_b, T, H, d.ln_eps, st)) return rc;
    if constexpr (std::is_void_v<GateAct>) {
        GemmParams g1 = gemm_16(b.x1, lw.up_w, lw.up_b, T, F, H);
        g1.C = b.act; g1.ldc = F;
        if (int rc = tt_gemm_launch(g1, TT_EPI_GELU, st)) return rc;
    } else {
        GemmParams g1 = gemm_16(b.x1, lw.up_w, lw.up_b, T, 2 * F, H);
        g1.C = b.gu; g1.ldc = 2 * F;
        if (int rc = tt_gemm_launch(g1, TT_EPI_BIAS, st)) return rc;
        if (int rc = gated_act_launch<GateAct>(b.gu, b.act, T, F, st)) return rc;
    }
    GemmParams g2 = gemm_16(b.act, lw.down_w, lw.down_b, T, H, F);
    g2.residual = b.x1; g2.ldr = H; g2.C = b.y; g2.ldc = H;
    if (int rc = tt_gemm_launch(g2, TT_EPI_RESIDUAL, st)) return rc;
    return postln_layernorm(b.y, out, lw.ln2_g, lw.ln2_b, T, H, d.ln_eps, st);
}

// the forward: hidden_out [n_rows][H] = the last layer's output (the embeddings of a model without layers)
template <class GateAct, class Family>
int postln_run(const PostLnDims& d, const Family& fam, const PackedSeqs& s, void* hidden_out, void* workspace, hipStream_t st) {
    TT_CHECK_ARG(d.gated == !std::is_void_v<GateAct>, "post-LN driver: the plan and the MLP disagree about the gate");
    const PostLnWs e = postln_plan(d, s.n_rows);
    char* ws = (char*)workspace;
    const auto at = [ws](size_t off) { return (uint16_t*)(ws + off); };
    const PostLnBufs b{at(e.off_x),   at(e.off_y),  at(e.off_x1),  at(e.off_qkv),
                       at(e.off_vt),  at(e.off_ctx), at(e.off_gu), at(e.off_act),
                       (const float*)(ws + e.off_zero), ws + e.off_tail};
    TT_CHECK_HIP(hipMemsetAsync(ws + e.off_zero, 0, d.zero_bytes, st));
    // rows that belong to no sequence are never written by the attention kernel: keep them finite
    TT_CHECK_HIP(hipMemsetAsync(b.ctx, 0, (size_t)s.n_rows * d.hidden * 2, st));
    uint16_t* x = d.layers == 0 ? (uint16_t*)hidden_out : b.x;
    {
        TtProfScope prof(TT_K_ROWOPS, st);
        if (int rc = fam.embed(b.zero, x, s.n_rows, st)) return rc;
    }
    for (int l = 0; l < d.layers; ++l) {
        // x1 is free again after the down-projection has consumed it as residual; the second LayerNorm's output goes back to x (or
        // straight to hidden_out on the last layer)
        uint16_t* dst = (l == d.layers - 1) ? (uint16_t*)hidden_out : x;
        if (int rc = postln_layer<GateAct>(d, fam, l, b, s, x, dst, st)) return rc;
        x = dst;
    }
    return TT_OK;
}

}  // namespace
