// EmbeddingGemma embedders (Gemma3TextModel with use_bidirectional_attention, e.g. google/embeddinggemma-300m): the whole-model
// forward, the sentence-transformers tail (mean pooling -> Dense -> Dense -> Normalize) and the kernels that only this family needs
// (include/tt_hip.h, "EmbeddingGemma embedders").  The projections run on the encoder's GEMMs (gemm.hip) with a zero bias and no
// residual in the epilogue: a post-norm sits between every projection and the residual stream.
//
// Layer schedule (four RMSNorms around two sublayers, no biases; one rounding to bf16 per stored tensor).  norm(v; w) is
// v * rsqrt(mean(v^2) + eps) * (1 + w):
//   h    = embed_tokens[ids] * bf16(sqrt(H))             [T][H]   before the first layer, with x = norm(h; input_layernorm of layer 0)
//   qkv  = GEMM(x, Wqkv)                                 [T][(nq + 2 nkv) D]  q_proj | k_proj | v_proj
//   qkv  = RoPE(norm_head(q; q_norm)), RoPE(norm_head(k; k_norm)) at the layer type's base, in place; V copied to the V8 layout vt
//   ctx  = bidirectional GQA attention(qkv, vt)          [T][nq D]   the shared tile (varlen.h attention_tile) with the window mask:
//                                                                    a sliding layer keeps |q - k| <= window, a full layer every key
//   y    = GEMM(ctx, Wo)                                 [T][H]
//   h1   = h + norm(y; post_attention_layernorm),  x = norm(h1; pre_feedforward_layernorm)        one fused row op
//   gu   = GEMM(x, [Wgate; Wup])                         [T][2F]
//   a    = GELU_tanh(gu[:, :F]) * gu[:, F:]              [T][F]
//   y    = GEMM(a, Wdown)                                [T][H]
//   h    = h1 + norm(y; post_feedforward_layernorm), x = norm(h; the next layer's input_layernorm)   the same row op; after the
//                                                        last layer the second norm is the model's final norm and x is hidden_out
// Every row op reads one token row only, so a token's result does not depend on how the batch is packed; the attention mixes the
// rows of one sequence only.  The layer loop below is this family's own: the sandwich norms produce the next layer's x inside the
// residual row op and the projections have no residual epilogue, so prenorm.h's two halves do not fit it.  The forward's prologue and
// buffers are prenorm.h's; the attention tile and its windowed wrapper, the gated-activation kernel with the tanh GELU, the
// workspace plan and the shape and batch-argument checks varlen.h's; the Dense tail pool_dense.h's.
//
// The row ops that add or subtract (h + norm(y), the rotation a cos - b sin) evaluate in fp64: where the two terms cancel, an fp32
// evaluation's own error (1e-7 of the terms) exceeds a bf16 ulp of the small result, and the parity tests hold every element to one
// ulp of the fp64 value.  These kernels move 5-6 KB per row; the arithmetic is a few hundred fp64 operations per lane, and the fused
// residual op still runs at two thirds of the copy bandwidth.
//
// bf16 only: the model card rules fp16 out (activations overflow), so this file is compiled once and has no _f16 twins.
#include "pool_dense.h"
#include "prenorm.h"

#include <cmath>

#if TT_F16
#error "gemma.hip is bf16 only"
#endif

namespace {

__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

__device__ __forceinline__ uint16_t f64_to_bf16_bits(double v) { return f32_to_bf16_bits((float)v); }

// ---- embedding gather with the embedding scale: out[r] = bf16(table[ids[r]] * scale) (an id outside [0, vocab): a zero row) -------
// The product of two bf16 values is exact in fp32, so this is the one rounding transformers' bf16 multiply makes.
__global__ __launch_bounds__(128) void gm_embed_kernel(const int32_t* __restrict__ ids, const uint16_t* __restrict__ table, int vocab,
                                                       int H, float scale, uint16_t* __restrict__ out) {
    const int row = blockIdx.x;
    const int id = ids[row];
    const bool ok = id >= 0 && id < vocab;
    const uint4* src = reinterpret_cast<const uint4*>(table + (size_t)(ok ? id : 0) * H);
    uint4* dst = reinterpret_cast<uint4*>(out + (size_t)row * H);
    for (int c = threadIdx.x; c < H / 8; c += blockDim.x) {
        if (!ok) {
            dst[c] = uint4{0u, 0u, 0u, 0u};
            continue;
        }
        const uint4 v = src[c];
        dst[c] = uint4{pack_e2(elo(v.x) * scale, ehi(v.x) * scale), pack_e2(elo(v.y) * scale, ehi(v.y) * scale),
                       pack_e2(elo(v.z) * scale, ehi(v.z) * scale), pack_e2(elo(v.w) * scale, ehi(v.w) * scale)};
    }
}

// ---- per-head RMSNorm of q and k with (1 + w), then rotate-half RoPE, in place; V heads copied to the V8 layout -------------------
// One block per token row, one wave per head at a time; heads of 256: lane l holds the pairs (l, l + 128) and (l + 64, l + 192).
//   angle = pos * inv[i], inv[i] = theta^(-2 i / 256) from the host (a kernel argument: 128 doubles)
//   out[i] = x[i] cos - x[i + 128] sin,  out[i + 128] = x[i + 128] cos + x[i] sin,  x = head * rsqrt(mean(head^2) + eps) * (1 + w)
struct GmRopeFreq {
    double inv[128];
};
__global__ __launch_bounds__(256) void gm_qknorm_rope_kernel(uint16_t* __restrict__ qkv, int ld, const int32_t* __restrict__ pos,
                                                             const float* __restrict__ qn, const float* __restrict__ kn, int nq, int nkv,
                                                             float eps, GmRopeFreq freq, uint16_t* __restrict__ vt, int ldvt) {
    constexpr int D = 256, half = 128;
    const int row = blockIdx.x;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const double p = (double)pos[row];
    uint16_t* r = qkv + (size_t)row * ld;
    // the row's 128 angles once per block (thread t < 128 evaluates angle t), shared by the four waves through LDS
    __shared__ double cos_sin[2][half];
    if (threadIdx.x < half) {
        double sn, cs;
        sincos(p * freq.inv[threadIdx.x], &sn, &cs);
        cos_sin[0][threadIdx.x] = cs;
        cos_sin[1][threadIdx.x] = sn;
    }
    __syncthreads();
    double c[2], s[2];
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        c[j] = cos_sin[0][lane + 64 * j];
        s[j] = cos_sin[1][lane + 64 * j];
    }
    for (int h = wave; h < nq + 2 * nkv; h += 4) {
        uint16_t* x = r + (size_t)h * D;
        if (h >= nq + nkv) {   // V head: vt[(row / 8) * ldvt + feature * 8 + row % 8]
            const size_t f0 = (size_t)(h - nq - nkv) * D;
            for (int d = lane; d < D; d += 64) vt[(size_t)(row >> 3) * ldvt + (f0 + d) * 8 + (row & 7)] = x[d];
            continue;
        }
        const float* g = h < nq ? qn : kn;
        double a[2], b[2], ss = 0.0;
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            a[j] = (double)bf16_bits_to_f32(x[lane + 64 * j]);
            b[j] = (double)bf16_bits_to_f32(x[lane + 64 * j + half]);
            ss += a[j] * a[j] + b[j] * b[j];
        }
        const double rs = 1.0 / sqrt(wave_sum_f64(ss) / (double)D + (double)eps);
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int i = lane + 64 * j;
            const double xa = a[j] * rs * (1.0 + (double)g[i]), xb = b[j] * rs * (1.0 + (double)g[i + half]);
            x[i] = f64_to_bf16_bits(xa * c[j] - xb * s[j]);
            x[i + half] = f64_to_bf16_bits(xb * c[j] + xa * s[j]);
        }
    }
}

// ---- the fused residual row op: h' = h + norm(y; wa), x' = norm(h'; wb); one wave per row of H <= 1024, four rows per block --------
// Both results come from the unrounded h' and are rounded once, as they are stored.  HAS_Y = false: the plain norm x' = norm(h; wb)
// in front of the first layer (and of a model without layers); nothing else is read or written.
template <bool HAS_Y>
__global__ __launch_bounds__(256) void gm_add_norm_kernel(const uint16_t* __restrict__ y, const uint16_t* __restrict__ h,
                                                          const float* __restrict__ wa, const float* __restrict__ wb, int rows, int H,
                                                          float eps, uint16_t* __restrict__ h_out, uint16_t* __restrict__ x_out) {
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    const int nc = H / 8;   // <= 128 chunks of 8 elements: at most two per lane
    const uint4 zero4 = uint4{0u, 0u, 0u, 0u};
    double hv[2][8];
    uint4 yv[2];
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int c = lane + 64 * j;
        const uint4 v = c < nc ? reinterpret_cast<const uint4*>(h + (size_t)row * H)[c] : zero4;
        if (HAS_Y) yv[j] = c < nc ? reinterpret_cast<const uint4*>(y + (size_t)row * H)[c] : zero4;
        const uint32_t u[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            hv[j][2 * k] = (double)elo(u[k]);
            hv[j][2 * k + 1] = (double)ehi(u[k]);
        }
    }
    if (HAS_Y) {
        double yd[2][8], ss = 0.0;
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const uint32_t u[4] = {yv[j].x, yv[j].y, yv[j].z, yv[j].w};
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                yd[j][2 * k] = (double)elo(u[k]);
                yd[j][2 * k + 1] = (double)ehi(u[k]);
                ss += yd[j][2 * k] * yd[j][2 * k];
                ss += yd[j][2 * k + 1] * yd[j][2 * k + 1];
            }
        }
        const double ra = 1.0 / sqrt(wave_sum_f64(ss) / (double)H + (double)eps);
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int c = lane + 64 * j;
            if (c >= nc) continue;
            uint32_t o[4];
#pragma unroll
            for (int k = 0; k < 8; ++k) hv[j][k] += yd[j][k] * ra * (1.0 + (double)wa[8 * c + k]);
#pragma unroll
            for (int k = 0; k < 4; ++k) o[k] = pack_bf16x2((float)hv[j][2 * k], (float)hv[j][2 * k + 1]);
            reinterpret_cast<uint4*>(h_out + (size_t)row * H)[c] = uint4{o[0], o[1], o[2], o[3]};
        }
    }
    double ss = 0.0;
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int k = 0; k < 8; ++k) ss += hv[j][k] * hv[j][k];   // (chunks past the row are zero)
    const double rb = 1.0 / sqrt(wave_sum_f64(ss) / (double)H + (double)eps);
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int c = lane + 64 * j;
        if (c >= nc) continue;
        uint32_t o[4];
#pragma unroll
        for (int k = 0; k < 4; ++k)
            o[k] = pack_bf16x2((float)(hv[j][2 * k] * rb * (1.0 + (double)wb[8 * c + 2 * k])),
                               (float)(hv[j][2 * k + 1] * rb * (1.0 + (double)wb[8 * c + 2 * k + 1])));
        reinterpret_cast<uint4*>(x_out + (size_t)row * H)[c] = uint4{o[0], o[1], o[2], o[3]};
    }
}

// ---- argument checks -----------------------------------------------------------------------------------------------------------
int check_heads(int heads, int kv_heads, int head_dim) { return check_gqa_heads("gemma", heads, kv_heads, head_dim, 256); }

int check_weights(const tt_gemma_weights* w) {
    TT_CHECK_ARG(w != nullptr, "null weights");
    if (int rc = check_heads(w->heads, w->kv_heads, w->head_dim)) return rc;
    if (int rc = check_hidden("gemma", w->hidden)) return rc;
    if (int rc = check_qkv_width("gemma", w->heads, w->kv_heads, w->head_dim, w->ffn)) return rc;
    TT_CHECK_ARG(w->layers >= 0 && (w->layers == 0 || w->layer != nullptr), "layer array missing");
    TT_CHECK_ARG(w->embed && w->final_norm && w->vocab > 0, "embedding table / final norm missing");
    TT_CHECK_ARG(w->rms_eps > 0.f && w->global_rope_theta > 0.f && w->local_rope_theta > 0.f && w->window >= 0 && w->embed_scale > 0.f,
                 "rms_eps=%g global_rope_theta=%g local_rope_theta=%g window=%d embed_scale=%g", w->rms_eps, w->global_rope_theta,
                 w->local_rope_theta, w->window, w->embed_scale);
    return TT_OK;
}

struct GemmaWs {
    VarlenWs e;
    size_t off_y, total;
};

GemmaWs gm_plan(const tt_gemma_weights* w, int n_rows) {
    const size_t H = (size_t)w->hidden, F = (size_t)w->ffn, D = (size_t)w->head_dim;
    const size_t nqkv = (size_t)(w->heads + 2 * w->kv_heads) * D;
    GemmaWs p{};
    // zeros: the GEMMs' bias operand (the model has none)
    p.e = varlen_plan(n_rows, H, nqkv, w->kv_heads * D, w->heads * D, 2 * F, F, std::max(nqkv, std::max(2 * F, H)));
    // y: the output of the two projections that feed a post-norm
    const size_t T = ((size_t)n_rows + 255) / 256 * 256;
    p.off_y = tt_align_up(p.e.total, 256);
    p.total = p.off_y + tt_align_up(T * H * 2, 256);
    return p;
}

int embed_launch(const int32_t* ids, const tt_gemma_weights* w, int rows, uint16_t* out, hipStream_t st) {
    TtProfScope prof(TT_K_ROWOPS, st);
    hipLaunchKernelGGL(gm_embed_kernel, dim3(rows), dim3(128), 0, st, ids, (const uint16_t*)w->embed, w->vocab, w->hidden, w->embed_scale,
                       out);
    TT_CHECK_LAUNCH();
    return TT_OK;
}

// y == nullptr: x_out = norm(h; wb) only
int add_norm_launch(const uint16_t* y, const uint16_t* h, const float* wa, const float* wb, int rows, int H, float eps, uint16_t* h_out,
                    uint16_t* x_out, hipStream_t st) {
    TtProfScope prof(TT_K_ROWOPS, st);
    if (y)
        hipLaunchKernelGGL(gm_add_norm_kernel<true>, dim3((rows + 3) / 4), dim3(256), 0, st, y, h, wa, wb, rows, H, eps, h_out, x_out);
    else
        hipLaunchKernelGGL(gm_add_norm_kernel<false>, dim3((rows + 3) / 4), dim3(256), 0, st, y, h, wa, wb, rows, H, eps, h_out, x_out);
    TT_CHECK_LAUNCH();
    return TT_OK;
}

int qknorm_rope_launch(uint16_t* qkv, int ld, const int32_t* pos, const float* qn, const float* kn, int rows, int nq, int nkv, float eps,
                       float theta, uint16_t* vt, int ldvt, hipStream_t st) {
    GmRopeFreq freq;
    for (int i = 0; i < 128; ++i) freq.inv[i] = pow((double)theta, -(double)(2 * i) / 256.0);
    TtProfScope prof(TT_K_ROWOPS, st);
    hipLaunchKernelGGL(gm_qknorm_rope_kernel, dim3(rows), dim3(256), 0, st, qkv, ld, pos, qn, kn, nq, nkv, eps, freq, vt, ldvt);
    TT_CHECK_LAUNCH();
    return TT_OK;
}

int gm_run(const tt_gemma_weights* w, const int32_t* ids, const int32_t* pos, const int32_t* seq_start, const int32_t* seq_len, int n_seq,
           int n_rows, int max_len, void* hidden_out, void* workspace, hipStream_t st) {
    const GemmaWs p = gm_plan(w, n_rows);
    const int H = w->hidden, F = w->ffn, D = w->head_dim, nq = w->heads, nkv = w->kv_heads, T = n_rows;
    const int nqkv = (nq + 2 * nkv) * D;
    VarlenBufs b;
    if (int rc = varlen_begin(p.e, workspace, T, nq * D, st, &b)) return rc;
    uint16_t* y = (uint16_t*)((char*)workspace + p.off_y);
    if (int rc = embed_launch(ids, w, T, b.ha, st)) return rc;
    if (w->layers == 0) return add_norm_launch(nullptr, b.ha, nullptr, w->final_norm, T, H, w->rms_eps, nullptr, (uint16_t*)hidden_out, st);
    if (int rc = add_norm_launch(nullptr, b.ha, nullptr, w->layer[0].input_norm, T, H, w->rms_eps, nullptr, b.x, st)) return rc;
    for (int l = 0; l < w->layers; ++l) {
        const tt_gemma_layer_weights& lw = w->layer[l];
        const bool last = l == w->layers - 1;
        GemmParams g = gemm_16(b.x, lw.qkv_w, b.zero, T, nqkv, H);
        g.C = b.qkv; g.ldc = nqkv;
        if (int rc = tt_gemm_launch(g, TT_EPI_BIAS, st)) return rc;
        if (int rc = qknorm_rope_launch(b.qkv, nqkv, pos, lw.q_norm, lw.k_norm, T, nq, nkv, w->rms_eps,
                                        lw.sliding ? w->local_rope_theta : w->global_rope_theta, b.vt, 8 * nkv * D, st))
            return rc;
        if (int rc = window_attention_launch<256>(b.qkv, nqkv, 0, nq * D, b.vt, 8 * nkv * D, b.ctx, nq * D, seq_start, seq_len, n_seq, T, nq, nkv,
                                                  max_len, lw.sliding ? w->window : -1, st))
            return rc;
        GemmParams go = gemm_16(b.ctx, lw.o_w, b.zero, T, H, nq * D);
        go.C = y; go.ldc = H;
        if (int rc = tt_gemm_launch(go, TT_EPI_BIAS, st)) return rc;
        if (int rc = add_norm_launch(y, b.ha, lw.post_attn_norm, lw.pre_ffn_norm, T, H, w->rms_eps, b.hb, b.x, st)) return rc;
        GemmParams g1 = gemm_16(b.x, lw.gate_up_w, b.zero, T, 2 * F, H);
        g1.C = b.gu; g1.ldc = 2 * F;
        if (int rc = tt_gemm_launch(g1, TT_EPI_BIAS, st)) return rc;
        if (int rc = gated_act_launch<GeluTanh>(b.gu, b.act, T, F, st)) return rc;
        GemmParams g2 = gemm_16(b.act, lw.down_w, b.zero, T, H, F);
        g2.C = y; g2.ldc = H;
        if (int rc = tt_gemm_launch(g2, TT_EPI_BIAS, st)) return rc;
        if (int rc = add_norm_launch(y, b.hb, lw.post_ffn_norm, last ? w->final_norm : w->layer[l + 1].input_norm, T, H, w->rms_eps, b.ha,
                                     last ? (uint16_t*)hidden_out : b.x, st))
            return rc;
    }
    return TT_OK;
}

}  // namespace

extern "C" {

size_t tt_gemma_workspace_bytes(const tt_gemma_weights* w, int n_rows) {
    if (!w || n_rows <= 0 || check_weights(w) != TT_OK) return 0;
    return gm_plan(w, n_rows).total;
}

int tt_gemma_forward(const tt_gemma_weights* w, const int32_t* ids, const int32_t* pos, const int32_t* type_ids, const int32_t* seq_start,
                     const int32_t* seq_len, int n_seq, int n_rows, int max_len, void* hidden_out, void* workspace,
                     size_t workspace_bytes, void* stream) {
    if (int rc = check_weights(w)) return rc;
    if (int rc = check_packed_forward_args("tt_gemma_forward", "EmbeddingGemma", ids, pos, type_ids, seq_start, seq_len, n_seq, n_rows,
                                           max_len, hidden_out, workspace, workspace_bytes, gm_plan(w, n_rows).total))
        return rc;
    for (int l = 0; l < w->layers; ++l) {
        const tt_gemma_layer_weights& lw = w->layer[l];
        TT_CHECK_ARG(lw.qkv_w && lw.q_norm && lw.k_norm && lw.o_w && lw.input_norm && lw.post_attn_norm && lw.pre_ffn_norm &&
                         lw.post_ffn_norm && lw.gate_up_w && lw.down_w,
                     "layer %d has a null weight pointer", l);
    }
    return gm_run(w, ids, pos, seq_start, seq_len, n_seq, n_rows, max_len, hidden_out, workspace, (hipStream_t)stream);
}

int tt_gemma_pool_dense(const tt_gemma_weights* w, const void* hidden, int ld, const int32_t* seq_start, const int32_t* seq_len,
                        int n_seq, float* out_f32, void* out_16, void* stream) {
    TT_CHECK_ARG(w != nullptr, "null weights");
    if (int rc = check_hidden("gemma", w->hidden)) return rc;
    TT_CHECK_ARG(n_seq >= 0, "n_seq=%d", n_seq);
    if (n_seq == 0) return TT_OK;
    TT_CHECK_ARG(hidden && seq_start && seq_len && out_f32, "null pointer");
    TT_CHECK_ARG(w->dense1_wt && w->dense2_wt, "these weights carry no Dense modules");
    if (w->dense1_out <= 0 || w->dense1_out % 64 || w->dense1_out > 3072 || w->dense2_out <= 0 || w->dense2_out % 64 ||
        w->dense2_out > 1024) {
        tt_set_error("gemma: Dense outputs %d and %d must be multiples of 64, up to 3072 and 1024 (the scan's limit)", w->dense1_out,
                     w->dense2_out);
        return TT_E_UNSUPPORTED;
    }
    TT_CHECK_ARG(ld >= w->hidden && ld % 8 == 0 && ((uintptr_t)hidden % 16) == 0, "hidden=%d ld=%d (16-byte aligned rows)", w->hidden, ld);
    // LDS: eight rows of max(hidden, dense2_out) + dense1_out floats, <= 128 KiB
    return pool_dense_launch(hidden, ld, seq_start, seq_len, n_seq, w->hidden, w->dense1_out, w->dense2_out, w->dense1_wt, w->dense2_wt,
                             out_f32, out_16, POOL_SB * (1024 + 3072) * sizeof(float), (hipStream_t)stream);
}

int tt_gemma_qk_norm_rope(void* qkv, int ld, const int32_t* pos, const float* q_norm, const float* k_norm, int n_rows, int heads,
                          int kv_heads, int head_dim, float eps, float rope_theta, void* vt, int ldvt, void* stream) {
    if (int rc = check_heads(heads, kv_heads, head_dim)) return rc;
    TT_CHECK_ARG(qkv && pos && q_norm && k_norm && vt, "null pointer");
    TT_CHECK_ARG(n_rows > 0 && n_rows % 8 == 0 && ld >= (heads + 2 * kv_heads) * head_dim && ldvt >= 8 * kv_heads * head_dim,
                 "n_rows=%d ld=%d ldvt=%d", n_rows, ld, ldvt);
    TT_CHECK_ARG(eps > 0.f && rope_theta > 0.f, "eps=%g rope_theta=%g", eps, rope_theta);
    return qknorm_rope_launch((uint16_t*)qkv, ld, pos, q_norm, k_norm, n_rows, heads, kv_heads, eps, rope_theta, (uint16_t*)vt, ldvt,
                              (hipStream_t)stream);
}

int tt_gemma_add_norm(const void* y, const void* h, const float* norm_a, const float* norm_b, int n_rows, int hidden, float eps,
                      void* h_out, void* x_out, void* stream) {
    if (int rc = check_hidden("gemma", hidden)) return rc;
    TT_CHECK_ARG(h && norm_b && x_out && n_rows > 0, "null pointer or n_rows=%d", n_rows);
    TT_CHECK_ARG(y == nullptr || (norm_a && h_out), "y without norm_a / h_out");
    TT_CHECK_ARG(eps > 0.f, "eps=%g", eps);
    TT_CHECK_ARG(((uintptr_t)y % 16) == 0 && ((uintptr_t)h % 16) == 0 && ((uintptr_t)h_out % 16) == 0 && ((uintptr_t)x_out % 16) == 0,
                 "rows must be 16-byte aligned");
    return add_norm_launch((const uint16_t*)y, (const uint16_t*)h, norm_a, norm_b, n_rows, hidden, eps, (uint16_t*)h_out, (uint16_t*)x_out,
                           (hipStream_t)stream);
}

int tt_attention_window_gqa(const void* qkv, int ld, int q_col0, int k_col0, const void* vt, int ldvt, void* out, int ld_out,
                            const int32_t* seq_start, const int32_t* seq_len, int n_seq, int n_rows, int heads, int kv_heads,
                            int head_dim, int max_len, int window, void* stream) {
    if (int rc = check_heads(heads, kv_heads, head_dim)) return rc;
    TT_CHECK_ARG(qkv && vt && out && seq_start && seq_len, "null pointer");
    TT_CHECK_ARG(n_seq > 0 && max_len > 0 && n_rows > 0 && n_rows % 8 == 0 && max_len <= n_rows, "n_seq=%d n_rows=%d max_len=%d", n_seq,
                 n_rows, max_len);
    TT_CHECK_ARG(ld % 8 == 0 && q_col0 % 8 == 0 && k_col0 % 8 == 0 && q_col0 >= 0 && k_col0 >= 0 && ld_out % 4 == 0 &&
                     ld >= std::max(q_col0 + heads * head_dim, k_col0 + kv_heads * head_dim) && ld_out >= heads * head_dim &&
                     ldvt >= 8 * kv_heads * head_dim && ldvt % 8 == 0,
                 "ld=%d q_col0=%d k_col0=%d ld_out=%d ldvt=%d", ld, q_col0, k_col0, ld_out, ldvt);
    return window_attention_launch<256>((const uint16_t*)qkv, ld, q_col0, k_col0, (const uint16_t*)vt, ldvt, (uint16_t*)out, ld_out,
                                        seq_start, seq_len, n_seq, n_rows, heads, kv_heads, max_len, window, (hipStream_t)stream);
}

}  // extern "C"
