// Decoder embedders and rerankers (Qwen3Model architecture: Qwen3-Embedding; Qwen3ForSequenceClassification): the whole-model
// forward, its pooled-row tail (the last layer for one row per sequence), last-token pooling, the score head and the kernels that
// only this family needs (include/tt_hip.h, "decoder embedder").  The projections run on the encoder's GEMMs (gemm.hip).
//
// Layer schedule (pre-norm block, no biases; one rounding to the element type per kernel output):
//   x    = RMSNorm(h) * g_attn                           [T][H]
//   qkv  = GEMM(x, Wqkv)                                 [T][(nq + 2 nkv) D]  q_proj | k_proj | v_proj
//   qkv  = RoPE(RMSNorm_head(q) * g_q), RoPE(RMSNorm_head(k) * g_k)   in place; V copied to the V8 layout vt
//   ctx  = causal GQA attention(qkv, vt)                 [T][nq D]   the shared tile (varlen.h attention_tile) with the causal mask
//   h1   = GEMM(ctx, Wo) + h                             residual fused in the epilogue
//   x    = RMSNorm(h1) * g_ffn
//   gu   = GEMM(x, [Wgate; Wup])                         [T][2F]
//   a    = SiLU(gu[:, :F]) * gu[:, F:]                   [T][F]
//   h    = GEMM(a, Wdown) + h1
// and after the last layer  out = RMSNorm(h) * g_final.  Every row op reads one token row only, so a token's result does not
// depend on how the batch is packed; the attention mixes the rows of one sequence only.  The schedule itself is prenorm.h's (the
// driver ModernBERT and T5 run on too: DecFamily below says what is Qwen3's); the attention tile, the embedding gather, RMSNorm, the
// gated-activation kernel, the workspace plan and the shape and batch-argument checks are varlen.h's.
//
// Compiled twice like the encoder path (common.h TT_F16): bf16 and fp16 (external names with an _f16 suffix, f16_names.h).
#include "prenorm.h"

namespace {

// ---- per-head RMSNorm of q and k with their weights, then rotate-half RoPE, in place; V heads copied to the V8 layout ---------
// One block per token row, one wave per head at a time; lane i < D / 2 holds the pair (i, i + D / 2).
//   inv_freq[i] = theta^(-2 i / D), angle = pos * inv_freq[i] (fp32, as transformers' default rotary embedding)
//   out[i] = x[i] cos - x[i + D/2] sin,  out[i + D/2] = x[i + D/2] cos + x[i] sin,  x = RMSNorm(head) * g
__global__ __launch_bounds__(256) void dec_qknorm_rope_kernel(uint16_t* __restrict__ qkv, int ld, const int32_t* __restrict__ pos,
                                                              const float* __restrict__ qn, const float* __restrict__ kn, int nq,
                                                              int nkv, int D, float eps, float theta, uint16_t* __restrict__ vt,
                                                              int ldvt) {
    const int row = blockIdx.x;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int half = D / 2;
    const float p = (float)pos[row];
    uint16_t* r = qkv + (size_t)row * ld;
    float c = 1.f, s = 0.f;
    if (lane < half) {
        const float inv = 1.0f / powf(theta, (float)(2 * lane) / (float)D);
        sincosf(p * inv, &s, &c);
    }
    for (int h = wave; h < nq + 2 * nkv; h += 4) {
        uint16_t* x = r + (size_t)h * D;
        if (h >= nq + nkv) {   // V head: vt[(row / 8) * ldvt + feature * 8 + row % 8]
            const size_t f0 = (size_t)(h - nq - nkv) * D;
            for (int d = lane; d < D; d += 64) vt[(size_t)(row >> 3) * ldvt + (f0 + d) * 8 + (row & 7)] = x[d];
            continue;
        }
        const float* g = h < nq ? qn : kn;
        float a = 0.f, b = 0.f;
        if (lane < half) {
            a = ebits_to_f32(x[lane]);
            b = ebits_to_f32(x[lane + half]);
        }
        const float rs = rsqrtf(wave_sum(a * a + b * b) / (float)D + eps);
        if (lane < half) {
            const float xa = a * rs * g[lane], xb = b * rs * g[lane + half];
            x[lane] = f32_to_ebits(xa * c - xb * s);
            x[lane + half] = f32_to_ebits(xb * c + xa * s);
        }
    }
}

// ---- last-token pooling + L2 norm: out[b] = h[r] / max(||h[r]||, 1e-12), r = seq_start[b] + seq_len[b] - 1; one wave per sequence
__global__ __launch_bounds__(256) void dec_pool_last_kernel(const uint16_t* __restrict__ hidden, int ld, const int32_t* __restrict__ seq_start,
                                                            const int32_t* __restrict__ seq_len, int n, int H, float* __restrict__ out,
                                                            uint16_t* __restrict__ out16) {
    const int lane = threadIdx.x & 63;
    const int b = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (b >= n) return;
    // an empty sequence has no last row (the row in front of it belongs to another sequence, or lies in front of the buffer): nothing
    // is read, and the zero vector comes out as it does for an all-zero row
    const bool any = seq_len[b] > 0;   // (wave-uniform)
    const int64_t r = any ? (int64_t)seq_start[b] + seq_len[b] - 1 : 0;
    const uint4* src = reinterpret_cast<const uint4*>(hidden + r * ld);
    const int nc = H / 8;
    uint4 v[2];
    float ss = 0.f;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int c = lane + 64 * j;
        v[j] = any && c < nc ? src[c] : uint4{0u, 0u, 0u, 0u};
        const uint32_t u[4] = {v[j].x, v[j].y, v[j].z, v[j].w};
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const float a = elo(u[k]), bb = ehi(u[k]);
            ss += a * a;
            ss += bb * bb;
        }
    }
    const float inv = 1.0f / fmaxf(sqrtf(wave_sum(ss)), 1e-12f);
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int c = lane + 64 * j;
        if (c >= nc) continue;
        const uint32_t u[4] = {v[j].x, v[j].y, v[j].z, v[j].w};
        float f[8];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            f[2 * k] = elo(u[k]) * inv;
            f[2 * k + 1] = ehi(u[k]) * inv;
        }
        float4* o = reinterpret_cast<float4*>(out + (size_t)b * H + 8 * c);
        o[0] = float4{f[0], f[1], f[2], f[3]};
        o[1] = float4{f[4], f[5], f[6], f[7]};
        if (out16)
            reinterpret_cast<uint4*>(out16 + (size_t)b * H)[c] =
                uint4{pack_e2(f[0], f[1]), pack_e2(f[2], f[3]), pack_e2(f[4], f[5]), pack_e2(f[6], f[7])};
    }
}

// ---- causal GQA attention over packed varlen sequences: one wave per (16-query tile, sequence, query head) on varlen.h's tile ------
template <int D>
__global__ __launch_bounds__(64) void dec_attention_kernel(const uint16_t* __restrict__ qkv, int ld, int q_col0, int k_col0,
                                                           const uint16_t* __restrict__ vt, int ldvt, uint16_t* __restrict__ out,
                                                           int ld_out, const int32_t* __restrict__ seq_start,
                                                           const int32_t* __restrict__ seq_len, int n_seq, int n_rows, int group,
                                                           int n_qt, float scale_log2) {
    const int t = n_qt - 1 - (int)blockIdx.x;   // the longest tiles (most keys) first
    for (int b = blockIdx.y; b < n_seq; b += gridDim.y)   // (wave-uniform: every lane takes the same sequences)
        attention_tile<D, false>(qkv, ld, q_col0, k_col0, vt, ldvt, out, ld_out, seq_start, seq_len, n_rows, group, 0, scale_log2, b,
                                 blockIdx.z, t);
}

// The pooled-row tail: per (sequence b, query head) only the 16-query tile that holds pool_row[b], and of it only that query,
// stored at compact row b of `out` [n_seq][ld_out].  A pool_row outside its sequence stores nothing (the row stays as it was).
template <int D>
__global__ __launch_bounds__(64) void dec_attention_rows_kernel(const uint16_t* __restrict__ qkv, int ld, int q_col0, int k_col0,
                                                                const uint16_t* __restrict__ vt, int ldvt, uint16_t* __restrict__ out,
                                                                int ld_out, const int32_t* __restrict__ seq_start,
                                                                const int32_t* __restrict__ seq_len,
                                                                const int32_t* __restrict__ pool_row, int n_seq, int n_rows,
                                                                int group, float scale_log2) {
    for (int b = blockIdx.x; b < n_seq; b += gridDim.x) {   // (wave-uniform)
        const int r = pool_row[b], s0 = seq_start[b], L = seq_len[b];
        if (s0 < 0 || r < s0 || r - s0 >= L || r >= n_rows) continue;
        attention_tile<D, false>(qkv, ld, q_col0, k_col0, vt, ldvt, out, ld_out, seq_start, seq_len, n_rows, group, 0, scale_log2, b,
                                 blockIdx.y, (r - s0) >> 4, r, b);
    }
}

// ---- gather of the pooled rows: dst[b] = src[rows[b]] for b < n (a row outside [0, n_rows) gives zeros), zeros up to n_pad ------
__global__ __launch_bounds__(256) void dec_gather_rows_kernel(const uint16_t* __restrict__ src, int ld, const int32_t* __restrict__ rows,
                                                              int n, int n_pad, int n_rows, int H, uint16_t* __restrict__ dst) {
    const int lane = threadIdx.x & 63;
    const int b = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (b >= n_pad) return;
    const int r = b < n ? rows[b] : -1;
    const bool ok = r >= 0 && r < n_rows;
    for (int c = lane; c < H / 8; c += 64)
        reinterpret_cast<uint4*>(dst + (size_t)b * H)[c] =
            ok ? reinterpret_cast<const uint4*>(src + (size_t)r * ld)[c] : uint4{0u, 0u, 0u, 0u};
}

// ---- score head of *ForSequenceClassification (one label, no bias): logit[b] = hidden[b] . w, score[b] = sigmoid(logit[b]) ------
// fp32 arithmetic, one wave per row; lane l sums the chunks l, l + 64 in ascending order, then the butterfly.
__global__ __launch_bounds__(256) void dec_score_kernel(const uint16_t* __restrict__ hidden, int ld, const float* __restrict__ w, int n,
                                                        int H, float* __restrict__ scores, float* __restrict__ logits) {
    const int lane = threadIdx.x & 63;
    const int b = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (b >= n) return;
    const uint4* src = reinterpret_cast<const uint4*>(hidden + (size_t)b * ld);
    float acc = 0.f;
    for (int c = lane; c < H / 8; c += 64) {
        const uint4 v = src[c];
        const uint32_t u[4] = {v.x, v.y, v.z, v.w};
        const float4 w0 = reinterpret_cast<const float4*>(w)[2 * c], w1 = reinterpret_cast<const float4*>(w)[2 * c + 1];
        acc += elo(u[0]) * w0.x;
        acc += ehi(u[0]) * w0.y;
        acc += elo(u[1]) * w0.z;
        acc += ehi(u[1]) * w0.w;
        acc += elo(u[2]) * w1.x;
        acc += ehi(u[2]) * w1.y;
        acc += elo(u[3]) * w1.z;
        acc += ehi(u[3]) * w1.w;
    }
    acc = wave_sum(acc);
    if (lane == 0) {
        scores[b] = 1.0f / (1.0f + expf(-acc));
        if (logits) logits[b] = acc;
    }
}

// ---- argument checks -----------------------------------------------------------------------------------------------------------
int check_heads(int heads, int kv_heads, int head_dim) { return check_gqa_heads("decoder", heads, kv_heads, head_dim, 64, 128); }

int check_weights(const tt_decoder_weights* w) {
    TT_CHECK_ARG(w != nullptr, "null weights");
    if (int rc = check_heads(w->heads, w->kv_heads, w->head_dim)) return rc;
    if (int rc = check_hidden("decoder", w->hidden)) return rc;
    if (int rc = check_qkv_width("decoder", w->heads, w->kv_heads, w->head_dim, w->ffn)) return rc;
    TT_CHECK_ARG(w->layers >= 0 && (w->layers == 0 || w->layer != nullptr), "layer array missing");
    TT_CHECK_ARG(w->embed && w->final_norm && w->vocab > 0, "embedding table / final norm missing");
    TT_CHECK_ARG(w->rms_eps > 0.f && w->rope_theta > 0.f, "rms_eps=%g rope_theta=%g", w->rms_eps, w->rope_theta);
    return TT_OK;
}

VarlenWs dec_plan(const tt_decoder_weights* w, int n_rows) {
    const size_t H = (size_t)w->hidden, F = (size_t)w->ffn, D = (size_t)w->head_dim;
    const size_t nqkv = (size_t)(w->heads + 2 * w->kv_heads) * D;
    // zeros: the GEMMs' bias operand (the model has none)
    return varlen_plan(n_rows, H, nqkv, w->kv_heads * D, w->heads * D, 2 * F, F, std::max(nqkv, std::max(2 * F, H)));
}

int qknorm_rope_launch(uint16_t* qkv, int ld, const int32_t* pos, const float* qn, const float* kn, int rows, int nq, int nkv, int D,
                       float eps, float theta, uint16_t* vt, int ldvt, hipStream_t st) {
    TtProfScope prof(TT_K_ROWOPS, st);
    hipLaunchKernelGGL(dec_qknorm_rope_kernel, dim3(rows), dim3(256), 0, st, qkv, ld, pos, qn, kn, nq, nkv, D, eps, theta, vt, ldvt);
    TT_CHECK_LAUNCH();
    return TT_OK;
}

int attention_launch(const uint16_t* qkv, int ld, int q_col0, int k_col0, const uint16_t* vt, int ldvt, uint16_t* out, int ld_out,
                     const int32_t* seq_start, const int32_t* seq_len, int n_seq, int n_rows, int heads, int kv_heads, int D,
                     int max_len, hipStream_t st) {
    const int n_qt = (max_len + 15) / 16;
    const dim3 grid(n_qt, std::min(n_seq, 65535), heads);   // more sequences: each block row takes every 65535th
    const float scale_log2 = 1.4426950408889634f / sqrtf((float)D);
    TtProfScope prof(TT_K_ATTENTION, st);
    if (D == 128)
        hipLaunchKernelGGL(dec_attention_kernel<128>, grid, dim3(64), 0, st, qkv, ld, q_col0, k_col0, vt, ldvt, out, ld_out, seq_start,
                           seq_len, n_seq, n_rows, heads / kv_heads, n_qt, scale_log2);
    else
        hipLaunchKernelGGL(dec_attention_kernel<64>, grid, dim3(64), 0, st, qkv, ld, q_col0, k_col0, vt, ldvt, out, ld_out, seq_start,
                           seq_len, n_seq, n_rows, heads / kv_heads, n_qt, scale_log2);
    TT_CHECK_LAUNCH();
    return TT_OK;
}

int attention_rows_launch(const uint16_t* qkv, int ld, int q_col0, int k_col0, const uint16_t* vt, int ldvt, uint16_t* out, int ld_out,
                          const int32_t* seq_start, const int32_t* seq_len, const int32_t* pool_row, int n_seq, int n_rows, int heads,
                          int kv_heads, int D, hipStream_t st) {
    const dim3 grid(std::min(n_seq, 1 << 20), heads);
    const float scale_log2 = 1.4426950408889634f / sqrtf((float)D);
    TtProfScope prof(TT_K_ATTENTION, st);
    if (D == 128)
        hipLaunchKernelGGL(dec_attention_rows_kernel<128>, grid, dim3(64), 0, st, qkv, ld, q_col0, k_col0, vt, ldvt, out, ld_out,
                           seq_start, seq_len, pool_row, n_seq, n_rows, heads / kv_heads, scale_log2);
    else
        hipLaunchKernelGGL(dec_attention_rows_kernel<64>, grid, dim3(64), 0, st, qkv, ld, q_col0, k_col0, vt, ldvt, out, ld_out,
                           seq_start, seq_len, pool_row, n_seq, n_rows, heads / kv_heads, scale_log2);
    TT_CHECK_LAUNCH();
    return TT_OK;
}

// rows of the compact buffers of the pooled-row tail: up to 256 sequences a multiple of 64 (the skinny GEMMs), else of 256
int rows_pad(int n_seq) { return pooled_rows_pad(n_seq, tt_gemm_skinny_enabled()); }

// what prenorm.h's driver asks of a family.  pool_row != nullptr (tt_decoder_forward_rows): the last layer's attention is the
// pooled-row one, into compact rows of b.ctx
struct DecFamily {
    static constexpr QkvForm qkv = QkvForm::Packed;
    const tt_decoder_weights* w;
    const int32_t *ids, *pos, *pool_row;

    int nqkv() const { return (w->heads + 2 * w->kv_heads) * w->head_dim; }
    PreNormDims dims() const { return {w->hidden, w->heads * w->head_dim, nqkv(), w->ffn, w->layers}; }
    int embed(const VarlenBufs& b, int T, hipStream_t st) const { return embed_gather_launch(ids, w->embed, w->vocab, w->hidden, b.ha, T, st); }
    int norm(const uint16_t* in, uint16_t* out, const float* g, const float*, int rows, hipStream_t st) const {
        return rmsnorm_launch<false>(in, out, g, rows, w->hidden, w->rms_eps, st);
    }
    PreNormLayer layer(int l) const {
        const tt_decoder_layer_weights& lw = w->layer[l];
        return {lw.attn_norm, lw.qkv_w, lw.o_w, lw.ffn_norm, lw.gate_up_w, lw.down_w};
    }
    int post_qkv(int l, const VarlenBufs& b, int T, hipStream_t st) const {
        return qknorm_rope_launch(b.qkv, nqkv(), pos, w->layer[l].q_norm, w->layer[l].k_norm, T, w->heads, w->kv_heads, w->head_dim,
                                  w->rms_eps, w->rope_theta, b.vt, 8 * w->kv_heads * w->head_dim, st);
    }
    int attention(int l, const VarlenBufs& b, const PackedSeqs& s, hipStream_t st) const {
        const int D = w->head_dim, nq = w->heads, nkv = w->kv_heads;
        if (pool_row && l == w->layers - 1) {
            TT_CHECK_HIP(hipMemsetAsync(b.ctx, 0, (size_t)rows_pad(s.n_seq) * nq * D * 2, st));
            return attention_rows_launch(b.qkv, nqkv(), 0, nq * D, b.vt, 8 * nkv * D, b.ctx, nq * D, s.seq_start, s.seq_len, pool_row,
                                         s.n_seq, s.n_rows, nq, nkv, D, st);
        }
        return attention_launch(b.qkv, nqkv(), 0, nq * D, b.vt, 8 * nkv * D, b.ctx, nq * D, s.seq_start, s.seq_len, s.n_seq, s.n_rows, nq,
                                nkv, D, s.max_len, st);
    }
    const float* final_norm() const { return w->final_norm; }
};

// The forward behind tt_decoder_forward (pool_row == nullptr: every layer over every row, out [n_rows][H]) and
// tt_decoder_forward_rows (the last layer's attention, output projection, MLP and the final norm for the rows pool_row names only,
// out [rows_pad(n_seq)][H]).  Arguments are checked by the callers.
int dec_run(const tt_decoder_weights* w, const int32_t* ids, const int32_t* pos, const int32_t* pool_row, const PackedSeqs& s,
            void* hidden_out, void* workspace, hipStream_t st) {
    const DecFamily fam{w, ids, pos, pool_row};
    const int H = w->hidden, T = s.n_rows, L = w->layers;
    VarlenBufs b;
    if (int rc = varlen_begin(dec_plan(w, T), workspace, T, w->heads * w->head_dim, st, &b)) return rc;
    if (!pool_row) return prenorm_run<Silu>(fam, b, s, hidden_out, st);
    if (int rc = fam.embed(b, T, st)) return rc;
    if (int rc = prenorm_layers<Silu>(fam, 0, L - 1, b, s, st)) return rc;
    // The last layer for the pooled rows only, on compact [M][...] buffers that reuse the full-size ones this layer no longer needs
    // (launches of one stream run in order): context -> ctx, residual rows of ha -> hb, h1 -> x, its norm -> ha, the layer's output
    // -> hb.  Rows n_seq .. M - 1 are zero and stay zero through every step.  A model without layers: embedding -> final norm of
    // the pooled rows.
    const int M = rows_pad(s.n_seq);
    if (L > 0)
        if (int rc = prenorm_attention_half(fam, L - 1, b, s, T, st)) return rc;
    {
        TtProfScope prof(TT_K_ROWOPS, st);
        hipLaunchKernelGGL(dec_gather_rows_kernel, dim3((M + 3) / 4), dim3(256), 0, st, b.ha, H, pool_row, s.n_seq, M, T, H, b.hb);
        TT_CHECK_LAUNCH();
    }
    if (L > 0)
        if (int rc = prenorm_tail_half<Silu>(fam, L - 1, b, M, b.ctx, b.hb, b.x, b.ha, b.hb, st)) return rc;
    return fam.norm(b.hb, (uint16_t*)hidden_out, w->final_norm, b.zero, M, st);
}

int check_forward_args(const char* what, const tt_decoder_weights* w, const int32_t* ids, const int32_t* pos, const int32_t* type_ids,
                       const int32_t* seq_start, const int32_t* seq_len, int n_seq, int n_rows, int max_len, const void* hidden_out,
                       const void* workspace, size_t workspace_bytes) {
    if (int rc = check_weights(w)) return rc;
    if (int rc = check_packed_forward_args(what, "a decoder", ids, pos, type_ids, seq_start, seq_len, n_seq, n_rows, max_len, hidden_out,
                                           workspace, workspace_bytes, dec_plan(w, n_rows).total))
        return rc;
    for (int l = 0; l < w->layers; ++l) {
        const tt_decoder_layer_weights& lw = w->layer[l];
        TT_CHECK_ARG(lw.qkv_w && lw.q_norm && lw.k_norm && lw.o_w && lw.attn_norm && lw.ffn_norm && lw.gate_up_w && lw.down_w,
                     "layer %d has a null weight pointer", l);
    }
    return TT_OK;
}

}  // namespace

extern "C" {

size_t tt_decoder_workspace_bytes(const tt_decoder_weights* w, int n_rows) {
    if (!w || n_rows <= 0 || check_weights(w) != TT_OK) return 0;
    return dec_plan(w, n_rows).total;
}

int tt_decoder_forward(const tt_decoder_weights* w, const int32_t* ids, const int32_t* pos, const int32_t* type_ids,
                       const int32_t* seq_start, const int32_t* seq_len, int n_seq, int n_rows, int max_len, void* hidden_out,
                       void* workspace, size_t workspace_bytes, void* stream) {
    if (int rc = check_forward_args("tt_decoder_forward", w, ids, pos, type_ids, seq_start, seq_len, n_seq, n_rows, max_len, hidden_out,
                                    workspace, workspace_bytes))
        return rc;
    return dec_run(w, ids, pos, nullptr, PackedSeqs{seq_start, seq_len, n_seq, n_rows, max_len}, hidden_out, workspace, (hipStream_t)stream);
}

size_t tt_decoder_rows_workspace_bytes(const tt_decoder_weights* w, int n_rows, int n_seq) {
    if (!w || n_rows <= 0 || n_seq <= 0 || n_seq > n_rows || check_weights(w) != TT_OK) return 0;
    return dec_plan(w, n_rows).total;   // the compact buffers of the tail reuse the full-size ones (rows_pad(n_seq) <= the padded n_rows)
}

int tt_decoder_forward_rows(const tt_decoder_weights* w, const int32_t* ids, const int32_t* pos, const int32_t* type_ids,
                            const int32_t* seq_start, const int32_t* seq_len, int n_seq, int n_rows, int max_len,
                            const int32_t* pool_row, void* hidden_out, void* workspace, size_t workspace_bytes, void* stream) {
    if (int rc = check_forward_args("tt_decoder_forward_rows", w, ids, pos, type_ids, seq_start, seq_len, n_seq, n_rows, max_len,
                                    hidden_out, workspace, workspace_bytes))
        return rc;
    TT_CHECK_ARG(pool_row != nullptr, "pool_row is NULL (one row per sequence)");
    TT_CHECK_ARG(n_seq <= n_rows, "n_seq=%d exceeds n_rows=%d", n_seq, n_rows);
    return dec_run(w, ids, pos, pool_row, PackedSeqs{seq_start, seq_len, n_seq, n_rows, max_len}, hidden_out, workspace, (hipStream_t)stream);
}

int tt_decoder_score(const void* hidden, int ld, const float* score_w, int n_seq, int hidden_size, float* scores, float* logits,
                     void* stream) {
    TT_CHECK_ARG(n_seq > 0, "n_seq=%d", n_seq);
    TT_CHECK_ARG(hidden && score_w && scores, "null pointer");
    TT_CHECK_ARG(hidden_size > 0 && hidden_size % 8 == 0 && hidden_size <= 1024 && ld >= hidden_size && ld % 8 == 0,
                 "hidden=%d ld=%d", hidden_size, ld);
    TT_CHECK_ARG(((uintptr_t)hidden % 16) == 0 && ((uintptr_t)score_w % 16) == 0, "hidden and score_w must be 16-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    TtProfScope prof(TT_K_ROWOPS, st);
    hipLaunchKernelGGL(dec_score_kernel, dim3((n_seq + 3) / 4), dim3(256), 0, st, (const uint16_t*)hidden, ld, score_w, n_seq,
                       hidden_size, scores, logits);
    TT_CHECK_LAUNCH();
    return TT_OK;
}

int tt_embed_pool_last(const void* hidden, int ld, const int32_t* seq_start, const int32_t* seq_len, int n_seq, int hidden_size,
                       float* out_f32, void* out_16, void* stream) {
    TT_CHECK_ARG(n_seq >= 0, "n_seq=%d", n_seq);
    if (n_seq == 0) return TT_OK;
    TT_CHECK_ARG(hidden && seq_start && seq_len && out_f32, "null pointer");
    TT_CHECK_ARG(ld >= hidden_size && ld % 8 == 0, "hidden=%d ld=%d", hidden_size, ld);
    if (hidden_size <= 0 || hidden_size % 8 || hidden_size > 1024) {   // (the code tt_embed_pool / tt_embed_pool_mean answer with)
        tt_set_error("tt_embed_pool_last: hidden size %d unsupported (multiple of 8, <= 1024)", hidden_size);
        return TT_E_UNSUPPORTED;
    }
    hipStream_t st = (hipStream_t)stream;
    TtProfScope prof(TT_K_ROWOPS, st);
    hipLaunchKernelGGL(dec_pool_last_kernel, dim3((n_seq + 3) / 4), dim3(256), 0, st, (const uint16_t*)hidden, ld, seq_start, seq_len,
                       n_seq, hidden_size, out_f32, (uint16_t*)out_16);
    TT_CHECK_LAUNCH();
    return TT_OK;
}

int tt_attention_causal_gqa(const void* qkv, int ld, int q_col0, int k_col0, const void* vt, int ldvt, void* out, int ld_out,
                            const int32_t* seq_start, const int32_t* seq_len, int n_seq, int n_rows, int heads, int kv_heads,
                            int head_dim, int max_len, void* stream) {
    if (int rc = check_heads(heads, kv_heads, head_dim)) return rc;
    TT_CHECK_ARG(qkv && vt && out && seq_start && seq_len, "null pointer");
    TT_CHECK_ARG(n_seq > 0 && max_len > 0 && n_rows > 0 && n_rows % 8 == 0 && max_len <= n_rows,
                 "n_seq=%d n_rows=%d max_len=%d", n_seq, n_rows, max_len);
    TT_CHECK_ARG(ld % 8 == 0 && q_col0 % 8 == 0 && k_col0 % 8 == 0 && ld_out % 4 == 0 && ldvt >= 8 * kv_heads * head_dim && ldvt % 8 == 0,
                 "ld=%d q_col0=%d k_col0=%d ld_out=%d ldvt=%d", ld, q_col0, k_col0, ld_out, ldvt);
    return attention_launch((const uint16_t*)qkv, ld, q_col0, k_col0, (const uint16_t*)vt, ldvt, (uint16_t*)out, ld_out, seq_start,
                            seq_len, n_seq, n_rows, heads, kv_heads, head_dim, max_len, (hipStream_t)stream);
}

int tt_qk_norm_rope(void* qkv, int ld, const int32_t* pos, const float* q_norm, const float* k_norm, int n_rows, int heads,
                    int kv_heads, int head_dim, float eps, float rope_theta, void* vt, int ldvt, void* stream) {
    if (int rc = check_heads(heads, kv_heads, head_dim)) return rc;
    TT_CHECK_ARG(qkv && pos && q_norm && k_norm && vt, "null pointer");
    TT_CHECK_ARG(n_rows > 0 && n_rows % 8 == 0 && ld >= (heads + 2 * kv_heads) * head_dim && ldvt >= 8 * kv_heads * head_dim,
                 "n_rows=%d ld=%d ldvt=%d", n_rows, ld, ldvt);
    TT_CHECK_ARG(eps > 0.f && rope_theta > 0.f, "eps=%g rope_theta=%g", eps, rope_theta);
    return qknorm_rope_launch((uint16_t*)qkv, ld, pos, q_norm, k_norm, n_rows, heads, kv_heads, head_dim, eps, rope_theta,
                              (uint16_t*)vt, ldvt, (hipStream_t)stream);
}

}  // extern "C"
