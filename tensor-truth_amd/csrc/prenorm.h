// The pre-norm block of the packed-varlen families, host side, written once (decoder.hip: Qwen3; modernbert.hip: ModernBERT; t5.hip:
// T5 encoders; and, for the prologue only, gemma.hip: EmbeddingGemma): the forward's prologue, the layer in two halves and the run
// function.  No device code here; the kernels are the encoder's (gemm.hip, rowops.hip, attention.hip), varlen.h's and the families'.
//
// Layer schedule (no biases: `zero` stands in; one rounding to the element type per kernel output):
//   x   = norm(h; attn_norm)                            [T][H]   skipped where the layer has none (ModernBERT's layer 0: x = h)
//   QkvForm::SplitV8:  qk, vT = QKV-GEMM(x)             [T][2H] + the V8 layout [T/8][H][8]                 (TT_EPI_QKV)
//   QkvForm::Packed:   qkv    = GEMM(x, Wqkv)           [T][qkv width]; the family's post-QKV step fills vT  (TT_EPI_BIAS)
//   the family's post-QKV step                          nothing, RoPE, or q/k-norm + RoPE -- in place
//   ctx = the family's attention(qkv, vT)               [T][q width]
//   ---- the tail half, on any number of rows ----
//   h1  = GEMM(ctx, Wo) + h                             residual fused in the epilogue                      (TT_EPI_RESIDUAL)
//   x   = norm(h1; ffn_norm)
//   GateAct void:      a  = relu(GEMM(x, Wup))          [T][F]                                              (TT_EPI_RELU)
//   GateAct an Act:    gu = GEMM(x, Wup)                [T][2F]                                             (TT_EPI_BIAS)
//                      a  = Act::f(gu[:, :F]) * gu[:, F:]                                                   (varlen.h gated_act_kernel<Act>)
//   h   = GEMM(a, Wdown) + h1                                                                               (TT_EPI_RESIDUAL)
// with h = the family's embedding launch before the first layer and out = norm(h; final_norm) behind the last.
//
// A family is a small struct the driver is a template over -- no allocation, no indirect call per launch:
//   static constexpr QkvForm qkv;
//   PreNormDims dims() const;
//   int embed(const VarlenBufs& b, int T, hipStream_t st) const;                               the embedding launch(es) -> b.ha
//   int norm(const uint16_t* in, uint16_t* out, const float* g, const float* zero, int rows, hipStream_t st) const;
//   PreNormLayer layer(int l) const;                                                           layer l's operands
//   int post_qkv(int l, const VarlenBufs& b, int T, hipStream_t st) const;                     b.qkv in place (+ b.vt)
//   int attention(int l, const VarlenBufs& b, const PackedSeqs& s, hipStream_t st) const;      b.qkv, b.vt -> b.ctx
//   const float* final_norm() const;
//
// EmbeddingGemma keeps its own layer loop (gemma.hip): its sandwich norms produce the next layer's x inside the residual row op
// and its projections have no residual epilogue, so neither half above is its half.  It takes the prologue, the buffers, the shape
// checks and the launches from here and from varlen.h.
#pragma once
#include "varlen.h"

#include <type_traits>

namespace {

// the carved workspace of a VarlenWs plan
struct VarlenBufs {
    uint16_t *ha, *hb, *x, *qkv, *vt, *ctx, *gu, *act;
    const float* zero;
};

// the prologue of every forward on a varlen_plan: carve the buffers, zero the zeros, and zero the n_rows x ctx_width context --
// rows that belong to no sequence are never written by the attention kernels: keep them finite (their V rows are masked keys)
inline int varlen_begin(const VarlenWs& e, void* workspace, int n_rows, int ctx_width, hipStream_t st, VarlenBufs* b) {
    char* ws = (char*)workspace;
    const auto at = [ws](size_t off) { return (uint16_t*)(ws + off); };
    *b = VarlenBufs{at(e.off_ha),  at(e.off_hb), at(e.off_x),  at(e.off_qkv), at(e.off_vt),
                    at(e.off_ctx), at(e.off_gu), at(e.off_act), (const float*)(ws + e.off_zero)};
    TT_CHECK_HIP(hipMemsetAsync(ws + e.off_zero, 0, e.zero_bytes, st));
    TT_CHECK_HIP(hipMemsetAsync(b->ctx, 0, (size_t)n_rows * ctx_width * 2, st));
    return TT_OK;
}

// one layer's operands, whatever the family calls them
struct PreNormLayer {
    const float* attn_norm;   // [H]; nullptr: the layer has none
    const void* qkv_w;        // [qkv width][H]
    const void* o_w;          // [H][q width]
    const float* ffn_norm;    // [H]
    const void* up_w;         // [F][H], or gated: [2F][H], the activated rows first
    const void* down_w;       // [H][F]
};

struct PreNormDims {
    int hidden, q_width, qkv_width, ffn, layers;   // q_width: heads * head_dim, the context's width; qkv_width: the projection's N
};

// the attention half on the batch's first `rows` rows: b.ha -> b.ctx (b.x, b.qkv and b.vt are scratch)
template <class Family>
int prenorm_attention_half(const Family& fam, int l, const VarlenBufs& b, const PackedSeqs& s, int rows, hipStream_t st) {
    const PreNormDims d = fam.dims();
    const PreNormLayer lw = fam.layer(l);
    const uint16_t* xin = b.ha;
    if (lw.attn_norm) {
        if (int rc = fam.norm(b.ha, b.x, lw.attn_norm, b.zero, rows, st)) return rc;
        xin = b.x;
    }
    GemmParams g = gemm_16(xin, lw.qkv_w, b.zero, rows, d.qkv_width, d.hidden);
    g.C = b.qkv;
    if constexpr (Family::qkv == QkvForm::SplitV8) {
        g.ldc = 2 * d.hidden; g.vt = b.vt; g.ldvt = 8 * d.hidden; g.vt_col0 = 2 * d.hidden;
        if (int rc = tt_gemm_launch(g, TT_EPI_QKV, st)) return rc;
    } else {
        g.ldc = d.qkv_width;
        if (int rc = tt_gemm_launch(g, TT_EPI_BIAS, st)) return rc;
    }
    if (int rc = fam.post_qkv(l, b, rows, st)) return rc;
    return fam.attention(l, b, s, st);
}

// the tail half on `rows` rows: the context `ctx` and the residual `res` through h1 and xn (and b.gu, b.act) into `out`
template <class GateAct, class Family>
int prenorm_tail_half(const Family& fam, int l, const VarlenBufs& b, int rows, const uint16_t* ctx, const uint16_t* res, uint16_t* h1,
                      uint16_t* xn, uint16_t* out, hipStream_t st) {
    const PreNormDims d = fam.dims();
    const PreNormLayer lw = fam.layer(l);
    const int H = d.hidden, F = d.ffn;
    GemmParams go = gemm_16(ctx, lw.o_w, b.zero, rows, H, d.q_width);
    go.residual = res; go.ldr = H; go.C = h1; go.ldc = H;
    if (int rc = tt_gemm_launch(go, TT_EPI_RESIDUAL, st)) return rc;
    if (int rc = fam.norm(h1, xn, lw.ffn_norm, b.zero, rows, st)) return rc;
    if constexpr (std::is_void_v<GateAct>) {
        GemmParams g1 = gemm_16(xn, lw.up_w, b.zero, rows, F, H);
        g1.C = b.act; g1.ldc = F;
        if (int rc = tt_gemm_launch(g1, TT_EPI_RELU, st)) return rc;
    } else {
        GemmParams g1 = gemm_16(xn, lw.up_w, b.zero, rows, 2 * F, H);
        g1.C = b.gu; g1.ldc = 2 * F;
        if (int rc = tt_gemm_launch(g1, TT_EPI_BIAS, st)) return rc;
        if (int rc = gated_act_launch<GateAct>(b.gu, b.act, rows, F, st)) return rc;
    }
    GemmParams g2 = gemm_16(b.act, lw.down_w, b.zero, rows, H, F);
    g2.residual = h1; g2.ldr = H; g2.C = out; g2.ldc = H;
    return tt_gemm_launch(g2, TT_EPI_RESIDUAL, st);
}

// the layers first .. last - 1 on every row: the residual stream stays in b.ha (h1 in b.hb, the normed rows in b.x)
template <class GateAct, class Family>
int prenorm_layers(const Family& fam, int first, int last, const VarlenBufs& b, const PackedSeqs& s, hipStream_t st) {
    for (int l = first; l < last; ++l) {
        if (int rc = prenorm_attention_half(fam, l, b, s, s.n_rows, st)) return rc;
        if (int rc = prenorm_tail_half<GateAct>(fam, l, b, s.n_rows, b.ctx, b.ha, b.hb, b.x, b.ha, st)) return rc;
    }
    return TT_OK;
}

// the forward behind a varlen_begin: hidden_out [n_rows][H] = norm(the last layer's output; final_norm)
template <class GateAct, class Family>
int prenorm_run(const Family& fam, const VarlenBufs& b, const PackedSeqs& s, void* hidden_out, hipStream_t st) {
    if (int rc = fam.embed(b, s.n_rows, st)) return rc;
    if (int rc = prenorm_layers<GateAct>(fam, 0, fam.dims().layers, b, s, st)) return rc;
    return fam.norm(b.ha, (uint16_t*)hidden_out, fam.final_norm(), b.zero, s.n_rows, st);
}

}  // namespace
