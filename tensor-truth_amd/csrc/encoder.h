// Internal interfaces of the encoder kernels (gemm.hip, attention.hip, rowops.hip, encoder_api.hip).
#pragma once
#include "common.h"
#include "gemm_plan.h"   // the TT_EPI_* epilogue ids

struct GemmParams {
    const uint16_t* A;        // [M][lda] bf16
    const uint16_t* W;        // [N][K] bf16 (nn.Linear weight)
    const float* bias;        // [N] fp32
    const uint16_t* residual; // [M][ldr] bf16 (TT_EPI_RESIDUAL)
    uint16_t* C;              // [M][ldc] bf16
    uint16_t* vt;             // TT_EPI_QKV: columns >= vt_col0 go to the V8 buffer:
                              //   vt[(m / 8) * ldvt + (n - vt_col0) * 8 + m % 8],  ldvt = 8 * (N - vt_col0)
    int M, N, K, lda, ldc, ldr, ldvt, vt_col0;
    // fp8 (OCP e4m3) operands: A, W point to bytes, lda / K count elements = bytes; the result is
    // acc * a_scale[m] * w_scale[n] (+ bias ...).  256x256 kernels only (bias, GELU and V^T epilogues).
    const float* a_scale;     // [M] per-row dequantisation scale of A
    const float* w_scale;     // [N] per-output-channel scale of W
    int fp8;
    // fp8 OUTPUT (bias / GELU epilogues of the one-tile kernel): C8[m][ldc] = e4m3(bf16(result) * c8_inv_scale),
    // one static scale for the whole tensor (the FFN intermediate, whose rows span 16 tiles); C is not written
    uint8_t* C8;
    float c8_inv_scale;
    int nt_store;             // whole-line output stores issued as streaming stores (set by the launcher)
    int sn;                   // super-tile width in N-tiles (32 tiles per super-tile: sm = 32 / sn); set by the launcher
    int scan_wave_lists;      // TT_EPI_SCAN, one-tile kernel: 1 = survivors go to wave-private LDS lists (set by tt_scan_gemm_launch).
                              // 0 or 1 only: gemm_kernel_v3 still tests bit 17 of this word on every A-tile address (gemm.hip stage_half)
    // TT_EPI_SCAN: candidate lists of the filter pass (same layout as ScanParams' shared lists)
    int32_t* scan_cnt;        // [N] running candidate count per query (may exceed scan_cap)
    float* scan_scores;       // [N][scan_cap]
    int32_t* scan_idx;        // [N][scan_cap]
    int scan_cap;
    int32_t scan_idx_base;    // emitted index = scan_idx_base + A row
    float* scan_dense;        // SAMPLE form (round 4): not null -> no filtering; tile t covers A rows [t * 256 * scan_tile_stride, + 256) and
    int scan_dense_stride;    // writes the maximum of each of its eight 32-row groups per query: scan_dense[q * stride + 8 t + group]
    int scan_tile_stride;
    int scan_rows;            // rows of the shard (0 = M).  Not a multiple of 256: M = rows rounded up, and the LAST tile is the
                              // shard's last 256 rows (it overlaps its predecessor; the rows scored twice are reported once)
    // ---- split-bf16 ("bf16x3") operands: reference precision on the bf16 matrix cores (x3_path.hip) -------------------
    // A value x is carried as TWO bf16 planes, hi = bf16(x) and lo = bf16(x - hi) (x = hi + lo to 2^-17 relative), stored
    // side by side in a row: A[m][0..K) = hi, A[m][K..2K) = lo (lda >= 2K), W[n][0..K) = hi, W[n][K..2K) = lo (ldw = 2K).
    // The product runs as ONE contraction over a virtual K' = 3K: A-hi.W-hi + A-hi.W-lo + A-lo.W-hi (lo.lo, 2^-16 of the
    // result, is dropped), fp32 accumulate -- the bf16 main loop unchanged, K-tile t reading A tile (t < nk ? t : t - nk)
    // and W tile (t < 2nk ? t : t - 2nk).  256x256 kernels only.  Epilogues: TT_EPI_BIAS / TT_EPI_GELU (exact erf) write
    // planes, C[m][n] = hi, C[m][c_lo_off + n] = lo; TT_EPI_RESIDUAL writes fp32, C32[m][n] = acc + bias + res32[m][n];
    // TT_EPI_VT writes the V8 layout twice (vt = hi, vt_lo = lo).
    int x3;
    int ldw;                  // W row stride in elements (0 = K)
    int c_lo_off;             // planes output: column offset of the lo plane
    float* C32;               // fp32 output [M][ldc] (x3 residual epilogue)
    const float* res32;       // fp32 residual [M][ldr]
    const uint16_t* res_planes;   // (round 4) the residual as the two planes of the same activation instead: res = hi + lo, hi at
    int res_lo_off;               // res_planes[m * ldr + n], lo res_lo_off columns further -- the LayerNorm then writes no fp32 copy
    uint16_t* vt_lo;          // lo plane of the V8 output
    int x3_zero_lo;           // diagnostic (TT_X3_ROUND_MASK): planes outputs are written with lo = 0, i.e. rounded to bf16
    // ---- f16c operands: reference precision on TWO matrix-time units (f16c_path.hip; fp16 instantiation only) ---------------
    // A value x is carried as "c-planes": hi = fp16(x), x8 = e4m3(x 2^-s), lo8 = e4m3((x - hi) 2^-(s - 11)), with one E8M0 block
    // exponent s per 32 consecutive K elements (s = exponent of the block's absmax - 7).  A row of an operand is ONE byte stream
    //     A[m]: [ hi: 2K bytes | x8: K | lo8: K ]        W[n]: [ hi: 2K | lo8: K | x8: K ]        (lda = ldw = 2K uint16 = 4K bytes)
    // and the product runs as ONE contraction over 2 K / 64 K-tiles of 128 bytes (K a multiple of 256): K / 64 tiles of v_mfma_f32_16x16x32_f16
    // (hi.hi), then K / 64 tiles of v_mfma_scale_f32_16x16x128_f8f6f4 with the block scales (x8.w_lo8, then lo8.w_x8): the cross
    // terms are 2^-12 of the result and need 2^-4, the dropped lo.lo term is 2^-24.  Scales are stored TILED, 1 KiB per (256-row
    // block, 128-element K-tile), in the order the kernel reads them (f16c_path.hip: a_scale_at / w_scale_at).
    // Epilogues: BIAS -> plain fp16 C (Q, K), VT -> fp16 V8, GELU -> c-planes (C = hi plane base, ldc = 2N uint16, c_scales),
    // RESIDUAL -> fp32 C32 = acc + bias + res32.
    int xc;
    const uint8_t* a_scales;  // [M / 256][K / 128][1024]
    const uint8_t* w_scales;  // [N / 256][2 K / 128][1024]: the w_lo8 part's K / 128 chunks, then the w_x8 part's (exponents - 11)
    uint8_t* c_scales;        // GELU epilogue: the output's scales, tiled for a consumer with K = N
};
// Filter pass of the similarity scan for 65..256 queries per pass as a 256x256x64-tiled MFMA contraction (gemm.hip):
// corpus [rows][dim] bf16 with rows a multiple of 256, queries256 [256][dim] bf16 (rows beyond the batch zero),
// thr256 [256] fp32 (+inf for rows beyond the batch).  ONE pass over the corpus whatever the batch size.
int tt_scan_gemm_launch(const uint16_t* corpus, int64_t rows, int dim, const uint16_t* queries256, const float* thr256,
                        int32_t* cnt, float* cand_scores, int32_t* cand_idx, int cap, int32_t idx_base, hipStream_t st);
// Threshold sample of the tiled scan on the same contraction: `tiles` row tiles of 256 rows, tile t at row t * 256 * tile_stride;
// dense[q * dense_stride + 8 t + g] = max over the tile's g-th 32-row group of q . row (NaN rows ignored).  One read of the sample
// rows for all 256 queries (the streaming sample kernel reads them once per 64-query tile).
int tt_scan_gemm_sample_launch(const uint16_t* corpus, int tiles, int tile_stride, int dim, const uint16_t* queries256, const float* thr256,
                               float* dense, int dense_stride, hipStream_t st);
int tt_gemm_launch(const GemmParams& p, int epilogue, hipStream_t st);
// M <= 256 (a multiple of 64) runs on the weight-streaming skinny kernel unless TT_GEMM_SKINNY=0 (A/B switch)
bool tt_gemm_skinny_enabled();

struct AttnParams {
    const uint16_t* qk;       // [T][ld_qk] bf16: Q at column q_col0 + h*dh, K at k_col0 + h*dh
    const uint16_t* vt;       // V8 layout [T/8][heads*dh][8] bf16: 8 consecutive tokens of one feature = 16 B;
                              // ldvt = elements per 8-token group = 8 * heads*dh
    uint16_t* out;            // [T][ld_out] bf16, context at column h*dh
    const int32_t* seq_start; // [B] first token row of each sequence (multiple of 8)
    const int32_t* seq_len;   // [B]
    int n_seq, heads, head_dim, max_len;
    int total_rows;           // token rows of the batch (0 = unknown): the launcher's wave-count choice wants the MEAN length too
    int ld_qk, q_col0, k_col0, ldvt, ld_out;
    float scale;              // 1/sqrt(head_dim)
    float lazy;               // set by the launcher: log2 slack of the running softmax reference
    int n_qt;                 // set by the launcher: query tiles per (sequence, head); workgroup L is tile L % n_qt of pair L / n_qt
    const uint16_t* q_rows;   // CLS variant only: the query row of sequence b at q_rows + b * ld_q_rows (+ h*dh); NULL = row seq_start[b] of qk
    int ld_q_rows;
    // f16c (fp16 instantiation): the context goes out as c-planes (f16c.h) -- `out` = the hi plane of rows of 4 * out_width bytes
    // (ld_out = 2 * out_width), x8 / lo8 planes behind it, block scales tiled for a consumer with K = out_width.  NULL = fp16 out.
    uint8_t* out_scales;
    int out_width;            // heads * head_dim
    int qk_lo_off;            // CLS variant, f16c: Q / K are TWO fp16 planes, the lo plane qk_lo_off columns behind the hi one (0 = one plane)
};
int tt_attention_launch(const AttnParams& p, hipStream_t st);
// key-limited variant (colbert.hip): every row of a sequence is a query, its first key_len[b] rows are the keys; sequences of up to
// 128 rows; reads qk, vt, out, seq_start, seq_len, n_seq, heads, head_dim, max_len, the strides and scale
int tt_attention_keylimit_launch(const AttnParams& p, const int32_t* key_len, hipStream_t st);
// CLS-only variant: one query row (seq_start[b]) per sequence; out row index = sequence index
int tt_attention_cls_launch(const AttnParams& p, hipStream_t st);

struct EmbedParams {
    const int32_t* ids;       // [T]
    const int32_t* pos;       // [T]
    const int32_t* type;      // [T] or null (=> type 0)
    const uint16_t* word;     // [vocab][H] bf16
    const uint16_t* posemb;   // [max_pos][H] bf16
    const uint16_t* typeemb;  // [type_vocab][H] bf16
    const float* gamma;
    const float* beta;
    uint16_t* out;            // [T][H] bf16
    int T, H, vocab, max_pos, type_vocab;
    float eps;
    uint8_t* q8;              // optional: [T][H] e4m3 copy of out, per-row scale q8_scale[T] (fp8 GEMM operand)
    float* q8_scale;
};
int tt_embed_ln_launch(const EmbedParams& p, hipStream_t st);

// out = LayerNorm(in) * gamma + beta, rows of H bf16
int tt_layernorm_launch(const uint16_t* in, uint16_t* out, const float* gamma, const float* beta, int rows, int H,
                        float eps, hipStream_t st, uint8_t* q8 = nullptr, float* q8_scale = nullptr);
int tt_absmax_launch(const uint16_t* x, size_t n, float* out, hipStream_t st);
int tt_quantize_rows_launch(const uint16_t* in, int ld, int rows, int cols, uint8_t* q8, float* scale, hipStream_t st);

// out_f32[b] = x[row[b]] / max(||x[row[b]]||, 1e-12); optional bf16 copy
int tt_cls_pool_l2norm_launch(const uint16_t* hidden, int ld, const int32_t* rows, int n, int H, float* out_f32,
                              uint16_t* out_bf16, hipStream_t st);

// gather rows: dst[b][:] = src[rows[b]][:]  (bf16, H elements), rows beyond n zero-filled up to n_pad
int tt_mean_pool_l2norm_launch(const void* hidden, int is_f32, int ld, const int32_t* seq_start, const int32_t* seq_len, int n, int H,
                               float* out_f32, uint16_t* out_bf16, hipStream_t st);
int tt_gather_rows_launch(const uint16_t* src, int ld, const int32_t* rows, int n, int n_pad, int H, uint16_t* dst,
                          hipStream_t st);

// score[b] = sigmoid(dot(t[b][:], w) + bias)   (t bf16 [n][ld], w bf16 [H]); logits optional
int tt_head_out_sigmoid_launch(const uint16_t* t, int ld, const uint16_t* w, const float* bias, int n, int H,
                               float* scores, float* logits, hipStream_t st);

// dist[i] = 1 - cos(e[i], e[i+1]), e fp32 [n][H]
int tt_adjacent_cosine_launch(const float* e, int n, int H, float* dist, hipStream_t st);

// fp32 rows: dst[b][0..H) = src[rows[b]][0..H) for b < n, zeros up to n_pad (f32_path.hip; the CLS tails of the split-plane
// and f16c forwards).  H a multiple of 4, both matrices [.][H].
int tt_gather_rows_f32_launch(const float* src, const int32_t* rows, int n, int n_pad, int H, float* dst, hipStream_t st);

// ---- host helpers of the forwards (encoder_api.hip, x3_path.hip, f16c_path.hip, f32_path.hip, decoder.hip) -------------------
// workspace layout: consecutive buffers, each starting on a 256-byte boundary
struct WsPlanner {
    size_t off = 0;
    size_t take(size_t bytes) { const size_t o = off; off += tt_align_up(bytes, 256); return o; }
};

// the workspace of entry point `what` is present, holds `need` bytes and is 256-byte aligned
inline int tt_check_workspace(const char* what, const void* workspace, size_t workspace_bytes, size_t need) {
    if (!workspace || workspace_bytes < need) {
        tt_set_error("%s: workspace %zu < required %zu bytes", what, workspace_bytes, need);
        return TT_E_WORKSPACE;
    }
    TT_CHECK_ARG(((uintptr_t)workspace % 256) == 0, "workspace must be 256-byte aligned");
    return TT_OK;
}

// Rows of the compact buffers a forward's last layer runs on when only one row per sequence is wanted (CLS tail, pooled rows):
// up to 256 sequences a multiple of 64 where the skinny GEMMs take them, else a multiple of 256 (the 256-row tile kernels).
// What the callers pass for skinny_allowed, and why:
//   bf16 / fp16 encoder, decoder: tt_gemm_skinny_enabled() -- with the diagnostic A/B switch off, the tile kernels need 256 rows;
//   split planes (x3):            true -- it has never consulted the switch (always on in the product library; with it off in the
//                                 diagnostic one, a tail of <= 192 rows is refused by the x3 GEMM launcher);
//   f16c:                         false -- the c-planes GEMM has no skinny kernel and its block scales are tiled per 256 rows.
inline int pooled_rows_pad(int n_seq, bool skinny_allowed) {
    return (n_seq <= 256 && skinny_allowed) ? (n_seq + 63) / 64 * 64 : (n_seq + 255) / 256 * 256;
}

// the classification head of the fp32-residual paths (x3, f16c) is a [n_seq x H x H] product: it runs on the fp32 kernels
// (tt_rerank_head_f32) through this view of the fp32 head weights
template <class Weights>
inline tt_encoder_weights_f32 head_weights_f32(const Weights* w) {
    tt_encoder_weights_f32 h{};
    h.hidden = w->hidden; h.layers = 0; h.heads = w->heads; h.ffn = w->ffn; h.vocab = w->vocab; h.max_pos = w->max_pos;
    h.type_vocab = w->type_vocab; h.ln_eps = w->ln_eps;
    h.word_emb = w->word_emb; h.pos_emb = w->pos_emb; h.type_emb = w->type_emb; h.emb_ln_g = w->emb_ln_g; h.emb_ln_b = w->emb_ln_b;
    h.cls_dense_w = w->cls_dense_w; h.cls_dense_b = w->cls_dense_b; h.cls_out_w = w->cls_out_w; h.cls_out_b = w->cls_out_b;
    return h;
}

// one projection on plain 16-bit operands: A [M][K], W [N][K] (the caller adds the epilogue's output and residual)
inline GemmParams gemm_16(const uint16_t* a, const void* w, const float* bias, int M, int N, int K) {
    GemmParams g{};
    g.A = a; g.lda = K; g.W = (const uint16_t*)w; g.bias = bias; g.M = M; g.N = N; g.K = K;
    return g;
}
