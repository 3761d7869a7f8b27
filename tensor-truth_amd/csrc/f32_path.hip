// Reference-precision (fp32) encoder forward, gfx950.
//
// The reference's DEFAULT embedder / reranker dtype is fp32 (app_utils/config_schema.py:66-76: torch_dtype None;
// services/model_manager.py:218-229 passes torch_dtype only when configured), and north_star's score tolerance --
// 1e-3 relative -- is an fp32 tolerance: the bf16 path rounds every activation to 8 significant bits 6 times per layer
// and lands at ~1e-2 on a sigmoid score after 24 layers.  This file is the path for callers who ask for
// model_kwargs={"torch_dtype": "float32"}: fp32 weights, fp32 activations, fp32 MFMA
// (v_mfma_f32_32x32x2_f32: exact f32 products and sums, 64 FLOP / clk / SIMD = 1/16 of the bf16 rate -- meant for
// the interactive case, one query's 50 pairs, not for bulk ingest).
//
// Kernels (all fp32 in / fp32 out):
//   embed_ln_f32      word + position + type embedding gather, LayerNorm            one wave per token row
//   gemm_f32<EPI>     C = epi(A . W^T + bias), 128 x 128 x 32 tiles, 4 waves of 64 x 64, operands staged through a
//                     padded LDS image (row stride 36 floats: conflict-free ds_read_b128), K order permuted inside
//                     groups of 8 (lane half h takes elements 4h..4h+3 for four consecutive MFMAs, both operands alike)
//   attention_f32     one query row per thread, keys / values streamed through LDS in tiles of 64, online softmax in
//                     sub-tiles of 16 keys; plain VALU FMAs (attention is < 5 % of the encoder's flops)
//   layernorm_f32, cls_pool_f32, head_out_f32
// Roofline: gemm_f32 is MFMA-bound at the fp32 matrix rate (157 TF/s peak); the rest is bandwidth- or VALU-bound and small.
#include "common.h"
#include "encoder.h"

namespace {

constexpr int kRowThreadsF = 256;   // 4 waves, one row per wave

// ---- LayerNorm of one row held as x[H/64] per lane (element e = lane + 64 * c) -------------------------------
template <int MAXC>
__device__ __forceinline__ void ln_row(float (&x)[MAXC], int nc, int H, const float* gamma, const float* beta, float eps,
                                       float* out, int lane) {
    float s = 0.f;
#pragma unroll
    for (int c = 0; c < MAXC; ++c)
        if (c < nc) s += x[c];
    const float mean = wave_sum(s) / (float)H;
    float v = 0.f;
#pragma unroll
    for (int c = 0; c < MAXC; ++c)
        if (c < nc) { const float d = x[c] - mean; v += d * d; }
    const float rstd = 1.0f / sqrtf(wave_sum(v) / (float)H + eps);
#pragma unroll
    for (int c = 0; c < MAXC; ++c)
        if (c < nc) {
            const int e = lane + 64 * c;
            out[e] = (x[c] - mean) * rstd * gamma[e] + beta[e];
        }
}

constexpr int kMaxC = 16;   // H <= 1024

__global__ __launch_bounds__(kRowThreadsF) void embed_ln_f32_kernel(const int32_t* ids, const int32_t* pos, const int32_t* type,
                                                                     const float* word, const float* posemb, const float* typeemb,
                                                                     const float* gamma, const float* beta, float* out, int T, int H,
                                                                     int vocab, int max_pos, int type_vocab, float eps) {
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (row >= T) return;
    int id, p, t;
    embed_rows_clamped(ids, pos, type, row, vocab, max_pos, type_vocab, id, p, t);
    const int nc = H / 64;
    float x[kMaxC];
#pragma unroll
    for (int c = 0; c < kMaxC; ++c)
        if (c < nc) {
            const int e = lane + 64 * c;
            x[c] = word[(size_t)id * H + e] + posemb[(size_t)p * H + e] + typeemb[(size_t)t * H + e];
        }
    ln_row<kMaxC>(x, nc, H, gamma, beta, eps, out + (size_t)row * H, lane);
}

__global__ __launch_bounds__(kRowThreadsF) void layernorm_f32_kernel(const float* in, float* out, const float* gamma, const float* beta,
                                                                      int rows, int H, float eps) {
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (row >= rows) return;
    const int nc = H / 64;
    float x[kMaxC];
#pragma unroll
    for (int c = 0; c < kMaxC; ++c)
        if (c < nc) x[c] = in[(size_t)row * H + lane + 64 * c];
    ln_row<kMaxC>(x, nc, H, gamma, beta, eps, out + (size_t)row * H, lane);
}

// ---- GEMM ---------------------------------------------------------------------------------------------------------
constexpr int FBM = 128, FBN = 128, FBK = 32;
constexpr int kLdF = FBK + 4;                       // padded row stride in floats (144 B): conflict-free b128 reads
constexpr int kTileF = FBM * kLdF * 4;              // 18 KiB per operand tile
constexpr int kGemmF32Lds = 4 * kTileF;             // A, W x 2 stages = 72 KiB (two workgroups per CU)

enum { F_EPI_BIAS = 0, F_EPI_GELU = 1, F_EPI_RESIDUAL = 2, F_EPI_TANH = 3 };

struct GemmF32Params {
    const float* A;   // [M][lda]
    const float* W;   // [N][K]
    const float* bias;
    const float* residual;   // [M][ldr]
    float* C;         // [M][ldc]
    int M, N, K, lda, ldc, ldr;
};

template <int EPI>
__global__ __launch_bounds__(256, 2) void gemm_f32_kernel(GemmF32Params p) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave >> 1, wn = wave & 1;
    const int m0 = blockIdx.y * FBM, n0 = blockIdx.x * FBN;
    const int nk = p.K / FBK;

    // staging: a tile is 128 rows x 8 float4; thread t loads float4 (row = t / 8 + 32 j, piece = t % 8), j = 0..3
    const int srow = tid >> 3, spiece = tid & 7;
    float4 ra[4], rw[4];
    auto gload = [&](int kt) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            int r = m0 + srow + 32 * j;
            r = r < p.M ? r : p.M - 1;                                  // tail rows: clamp (never stored)
            ra[j] = *reinterpret_cast<const float4*>(p.A + (size_t)r * p.lda + kt * FBK + spiece * 4);
            rw[j] = *reinterpret_cast<const float4*>(p.W + (size_t)(n0 + srow + 32 * j) * p.K + kt * FBK + spiece * 4);
        }
    };
    auto swrite = [&](int stage) {
        float* ta = reinterpret_cast<float*>(smem + stage * 2 * kTileF);
        float* tw = reinterpret_cast<float*>(smem + stage * 2 * kTileF + kTileF);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            *reinterpret_cast<float4*>(ta + (srow + 32 * j) * kLdF + spiece * 4) = ra[j];
            *reinterpret_cast<float4*>(tw + (srow + 32 * j) * kLdF + spiece * 4) = rw[j];
        }
    };

    f32x16 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

    gload(0);
    swrite(0);
    __syncthreads();
    const int fr = lane & 31, fh = lane >> 5;
    for (int kt = 0; kt < nk; ++kt) {
        const int st = kt & 1;
        if (kt + 1 < nk) gload(kt + 1);
        const float* ta = reinterpret_cast<const float*>(smem + st * 2 * kTileF);
        const float* tw = reinterpret_cast<const float*>(smem + st * 2 * kTileF + kTileF);
#pragma unroll
        for (int g8 = 0; g8 < FBK / 8; ++g8) {
            float4 af[2], wf[2];
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                af[i] = *reinterpret_cast<const float4*>(ta + (wm * 64 + i * 32 + fr) * kLdF + g8 * 8 + fh * 4);
                wf[i] = *reinterpret_cast<const float4*>(tw + (wn * 64 + i * 32 + fr) * kLdF + g8 * 8 + fh * 4);
            }
#pragma unroll
            for (int kk = 0; kk < 4; ++kk) {
                const float a0 = kk == 0 ? af[0].x : kk == 1 ? af[0].y : kk == 2 ? af[0].z : af[0].w;
                const float a1 = kk == 0 ? af[1].x : kk == 1 ? af[1].y : kk == 2 ? af[1].z : af[1].w;
                const float w0 = kk == 0 ? wf[0].x : kk == 1 ? wf[0].y : kk == 2 ? wf[0].z : wf[0].w;
                const float w1 = kk == 0 ? wf[1].x : kk == 1 ? wf[1].y : kk == 2 ? wf[1].z : wf[1].w;
                acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, w0, acc[0][0], 0, 0, 0);
                acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, w1, acc[0][1], 0, 0, 0);
                acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, w0, acc[1][0], 0, 0, 0);
                acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, w1, acc[1][1], 0, 0, 0);
            }
        }
        if (kt + 1 < nk) swrite(st ^ 1);
        __syncthreads();
    }

    // epilogue: lane holds output column n = lane & 31 of a 32-wide tile and rows (r & 3) + 8 (r >> 2) + 4 (lane >> 5)
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int n = n0 + wn * 64 + j * 32 + fr;
        const float b = p.bias[n];
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int m = m0 + wm * 64 + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * fh;
                if (m < p.M) {
                    float v = acc[i][j][r] + b;
                    if constexpr (EPI == F_EPI_GELU) v = 0.5f * v * (1.0f + erff(v * 0.70710678118654752f));
                    else if constexpr (EPI == F_EPI_TANH) v = tanhf(v);
                    else if constexpr (EPI == F_EPI_RESIDUAL) v += p.residual[(size_t)m * p.ldr + n];
                    p.C[(size_t)m * p.ldc + n] = v;
                }
            }
    }
}

template <int EPI>
int launch_gemm_f32(const GemmF32Params& p, hipStream_t st) {
    TT_SET_MAX_LDS(gemm_f32_kernel<EPI>, kGemmF32Lds);
    hipLaunchKernelGGL(gemm_f32_kernel<EPI>, dim3(p.N / FBN, (p.M + FBM - 1) / FBM), dim3(256), kGemmF32Lds, st, p);
    TT_CHECK_LAUNCH();
    return TT_OK;
}

int gemm_f32(const GemmF32Params& p, int epi, hipStream_t st) {
    if (p.M <= 0) return TT_OK;
    if (p.N % FBN || p.K % FBK || p.K <= 0 || p.lda % 4 || p.K % 4) {
        tt_set_error("gemm_f32: N=%d must be a multiple of 128 and K=%d of 32", p.N, p.K);
        return TT_E_UNSUPPORTED;
    }
    TtProfScope prof(TT_K_GEMM, st);
    switch (epi) {
        case F_EPI_BIAS: return launch_gemm_f32<F_EPI_BIAS>(p, st);
        case F_EPI_GELU: return launch_gemm_f32<F_EPI_GELU>(p, st);
        case F_EPI_RESIDUAL: return launch_gemm_f32<F_EPI_RESIDUAL>(p, st);
        default: return launch_gemm_f32<F_EPI_TANH>(p, st);
    }
}

// ---- attention ---------------------------------------------------------------------------------------------------
// grid (query blocks of 128 rows, heads, sequences); 128 threads, one query row each.  qkv: [T][3H] fp32.
constexpr int kAttKT = 64;     // keys per LDS tile
constexpr int kAttSub = 16;    // keys per softmax step

template <int DH>
__global__ __launch_bounds__(128) void attention_f32_kernel(const float* qkv, float* out, const int32_t* seq_start,
                                                             const int32_t* seq_len, int H, float scale) {
    __shared__ __attribute__((aligned(16))) float kt[kAttKT][DH];
    __shared__ __attribute__((aligned(16))) float vt[kAttKT][DH];
    const int b = blockIdx.z, h = blockIdx.y;
    const int len = seq_len[b], start = seq_start[b];
    const int q_row = blockIdx.x * 128 + threadIdx.x;
    if (blockIdx.x * 128 >= len) return;                      // whole block beyond the sequence (block-uniform)
    const bool active = q_row < len;
    const int ld = 3 * H;
    float q[DH], o[DH];
    {
        const float* qp = qkv + (size_t)(start + (active ? q_row : 0)) * ld + h * DH;
#pragma unroll
        for (int d = 0; d < DH; d += 4) {
            const float4 v = *reinterpret_cast<const float4*>(qp + d);
            q[d] = v.x * scale; q[d + 1] = v.y * scale; q[d + 2] = v.z * scale; q[d + 3] = v.w * scale;
        }
    }
#pragma unroll
    for (int d = 0; d < DH; ++d) o[d] = 0.f;
    float m = -__builtin_inff(), l = 0.f;
    for (int k0 = 0; k0 < len; k0 += kAttKT) {
        const int nk = (len - k0) < kAttKT ? (len - k0) : kAttKT;
        __syncthreads();
        for (int i = threadIdx.x; i < kAttKT * DH / 4; i += 128) {
            const int r = i / (DH / 4), c = (i % (DH / 4)) * 4;
            float4 kv = make_float4(0.f, 0.f, 0.f, 0.f), vv = kv;
            if (r < nk) {
                const float* base = qkv + (size_t)(start + k0 + r) * ld + h * DH + c;
                kv = *reinterpret_cast<const float4*>(base + H);
                vv = *reinterpret_cast<const float4*>(base + 2 * H);
            }
            *reinterpret_cast<float4*>(&kt[r][c]) = kv;
            *reinterpret_cast<float4*>(&vt[r][c]) = vv;
        }
        __syncthreads();
        for (int s0 = 0; s0 < nk; s0 += kAttSub) {
            float s[kAttSub];
            float mx = -__builtin_inff();
#pragma unroll
            for (int j = 0; j < kAttSub; ++j) {
                float acc = 0.f;
#pragma unroll
                for (int d = 0; d < DH; d += 4) {
                    const float4 kv = *reinterpret_cast<const float4*>(&kt[s0 + j][d]);     // same address in every lane: broadcast
                    acc = fmaf(q[d], kv.x, acc); acc = fmaf(q[d + 1], kv.y, acc);
                    acc = fmaf(q[d + 2], kv.z, acc); acc = fmaf(q[d + 3], kv.w, acc);
                }
                s[j] = (s0 + j < nk) ? acc : -__builtin_inff();
                mx = fmaxf(mx, s[j]);
            }
            const float m_new = fmaxf(m, mx);
            const float alpha = expf(m - m_new);            // m = -inf on the first step: exp(-inf) = 0
            l *= alpha;
#pragma unroll
            for (int d = 0; d < DH; ++d) o[d] *= alpha;
#pragma unroll
            for (int j = 0; j < kAttSub; ++j) {
                const float pj = expf(s[j] - m_new);        // masked keys: exp(-inf) = 0
                l += pj;
#pragma unroll
                for (int d = 0; d < DH; d += 4) {
                    const float4 vv = *reinterpret_cast<const float4*>(&vt[s0 + j][d]);
                    o[d] = fmaf(pj, vv.x, o[d]); o[d + 1] = fmaf(pj, vv.y, o[d + 1]);
                    o[d + 2] = fmaf(pj, vv.z, o[d + 2]); o[d + 3] = fmaf(pj, vv.w, o[d + 3]);
                }
            }
            m = m_new;
        }
    }
    if (active) {
        const float inv = 1.0f / l;
        float* op = out + (size_t)(start + q_row) * H + h * DH;
#pragma unroll
        for (int d = 0; d < DH; d += 4)
            *reinterpret_cast<float4*>(op + d) = make_float4(o[d] * inv, o[d + 1] * inv, o[d + 2] * inv, o[d + 3] * inv);
    }
}

// ---- pooling / head ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kRowThreadsF) void cls_pool_f32_kernel(const float* hidden, int ld, const int32_t* rows, int n, int H,
                                                                     float* out_f32, uint16_t* out_bf16) {
    const int b = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (b >= n) return;
    const float* x = hidden + (size_t)rows[b] * ld;
    float ss = 0.f;
    for (int e = lane; e < H; e += 64) ss += x[e] * x[e];
    const float inv = 1.0f / fmaxf(sqrtf(wave_sum(ss)), 1e-12f);
    for (int e = lane; e < H; e += 64) {
        const float v = x[e] * inv;
        out_f32[(size_t)b * H + e] = v;
        if (out_bf16) out_bf16[(size_t)b * H + e] = f32_to_bf16_bits(v);
    }
}

__global__ __launch_bounds__(kRowThreadsF) void gather_rows_f32_kernel(const float* src, int ld, const int32_t* rows, int n, int n_pad, int H,
                                                                        float* dst) {
    const int b = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (b >= n_pad) return;
    for (int e = lane; e < H; e += 64) dst[(size_t)b * H + e] = b < n ? src[(size_t)rows[b] * ld + e] : 0.f;
}

// the same gather, one workgroup per row in float4 pieces, both matrices [.][H] (tt_gather_rows_f32_launch: the CLS tails of the
// split-plane and f16c forwards)
__global__ __launch_bounds__(256) void gather_rows_f32x4_kernel(const float* src, const int32_t* rows, int n, int n_pad, int H, float* dst) {
    const int b = blockIdx.x;
    if (b >= n_pad) return;
    for (int c = threadIdx.x * 4; c < H; c += 256 * 4) {
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (b < n) v = *reinterpret_cast<const float4*>(src + (size_t)rows[b] * H + c);
        *reinterpret_cast<float4*>(dst + (size_t)b * H + c) = v;
    }
}

__global__ __launch_bounds__(kRowThreadsF) void head_out_f32_kernel(const float* t, int ld, const float* w, const float* bias, int n, int H,
                                                                     float* scores, float* logits) {
    const int b = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (b >= n) return;
    float s = 0.f;
    for (int e = lane; e < H; e += 64) s = fmaf(t[(size_t)b * ld + e], w[e], s);
    s = wave_sum(s) + bias[0];
    if (lane == 0) {
        if (logits) logits[b] = s;
        scores[b] = 1.0f / (1.0f + expf(-s));
    }
}

struct F32Ws {
    size_t off_xa, off_xb, off_y, off_qkv, off_ctx, off_ffn, total;
};

F32Ws f32_plan(const tt_encoder_weights_f32* w, int n_rows) {
    F32Ws e{};
    const size_t H = (size_t)w->hidden, F = (size_t)w->ffn, T = (size_t)n_rows;
    WsPlanner ws;
    e.off_xa = ws.take(T * H * 4);
    e.off_xb = ws.take(T * H * 4);
    e.off_y = ws.take(T * H * 4);
    e.off_qkv = ws.take(T * 3 * H * 4);
    e.off_ctx = ws.take(T * H * 4);
    e.off_ffn = ws.take(T * F * 4);
    e.total = ws.off;
    return e;
}

int check_weights_f32(const tt_encoder_weights_f32* w) {
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

inline dim3 row_grid_f(int rows) { return dim3((unsigned)((rows + 3) / 4)); }

}  // namespace

int tt_gather_rows_f32_launch(const float* src, const int32_t* rows, int n, int n_pad, int H, float* dst, hipStream_t st) {
    TtProfScope prof(TT_K_ROWOPS, st);
    hipLaunchKernelGGL(gather_rows_f32x4_kernel, dim3(n_pad), dim3(256), 0, st, src, rows, n, n_pad, H, dst);
    TT_CHECK_LAUNCH();
    return TT_OK;
}

extern "C" {

size_t tt_encoder_f32_workspace_bytes(const tt_encoder_weights_f32* w, int n_rows) {
    if (!w || n_rows <= 0) return 0;
    return f32_plan(w, n_rows).total;
}

int tt_encoder_forward_f32(const tt_encoder_weights_f32* w, const int32_t* ids, const int32_t* pos, const int32_t* type_ids,
                           const int32_t* seq_start, const int32_t* seq_len, int n_seq, int n_rows, int max_len,
                           float* hidden_out, void* workspace, size_t workspace_bytes, void* stream) {
    if (int rc = check_weights_f32(w)) return rc;
    TT_CHECK_ARG(n_rows > 0 && n_seq > 0 && max_len > 0, "n_rows=%d n_seq=%d max_len=%d", n_rows, n_seq, max_len);
    TT_CHECK_ARG(ids && pos && seq_start && seq_len && hidden_out, "null pointer");
    const F32Ws e = f32_plan(w, n_rows);
    if (int rc = tt_check_workspace("tt_encoder_forward_f32", workspace, workspace_bytes, e.total)) return rc;
    hipStream_t st = (hipStream_t)stream;
    char* ws = (char*)workspace;
    const int H = w->hidden, F = w->ffn, T = n_rows, dh = H / w->heads;
    float* xa = (float*)(ws + e.off_xa);
    float* xb = (float*)(ws + e.off_xb);
    float* y = (float*)(ws + e.off_y);
    float* qkv = (float*)(ws + e.off_qkv);
    float* ctx = (float*)(ws + e.off_ctx);
    float* ffn = (float*)(ws + e.off_ffn);
    TT_CHECK_HIP(hipMemsetAsync(ctx, 0, (size_t)T * H * 4, st));     // rows of no sequence are never written by attention
    float* x = w->layers == 0 ? hidden_out : xa;
    {
        TtProfScope prof(TT_K_ROWOPS, st);
        hipLaunchKernelGGL(embed_ln_f32_kernel, row_grid_f(T), dim3(kRowThreadsF), 0, st, ids, pos, type_ids, w->word_emb, w->pos_emb,
                           w->type_emb, w->emb_ln_g, w->emb_ln_b, x, T, H, w->vocab, w->max_pos, w->type_vocab, w->ln_eps);
        TT_CHECK_LAUNCH();
    }
    const float scale = 1.0f / sqrtf((float)dh);
    for (int l = 0; l < w->layers; ++l) {
        const tt_layer_weights_f32& lw = w->layer[l];
        TT_CHECK_ARG(lw.qkv_w && lw.qkv_b && lw.o_w && lw.o_b && lw.ln1_g && lw.ln1_b && lw.ffn1_w && lw.ffn1_b && lw.ffn2_w &&
                         lw.ffn2_b && lw.ln2_g && lw.ln2_b, "layer %d has a null weight pointer", l);
        GemmF32Params g{};
        g.A = x; g.lda = H; g.W = lw.qkv_w; g.bias = lw.qkv_b; g.C = qkv; g.ldc = 3 * H; g.M = T; g.N = 3 * H; g.K = H;
        if (int rc = gemm_f32(g, F_EPI_BIAS, st)) return rc;
        {
            TtProfScope prof(TT_K_ATTENTION, st);
            const dim3 grid((unsigned)((max_len + 127) / 128), (unsigned)w->heads, (unsigned)n_seq);
            if (dh == 64) hipLaunchKernelGGL(attention_f32_kernel<64>, grid, dim3(128), 0, st, qkv, ctx, seq_start, seq_len, H, scale);
            else hipLaunchKernelGGL(attention_f32_kernel<32>, grid, dim3(128), 0, st, qkv, ctx, seq_start, seq_len, H, scale);
            TT_CHECK_LAUNCH();
        }
        GemmF32Params go{};
        go.A = ctx; go.lda = H; go.W = lw.o_w; go.bias = lw.o_b; go.residual = x; go.ldr = H; go.C = y; go.ldc = H;
        go.M = T; go.N = H; go.K = H;
        if (int rc = gemm_f32(go, F_EPI_RESIDUAL, st)) return rc;
        float* x1 = (x == xa) ? xb : xa;
        {
            TtProfScope prof(TT_K_ROWOPS, st);
            hipLaunchKernelGGL(layernorm_f32_kernel, row_grid_f(T), dim3(kRowThreadsF), 0, st, y, x1, lw.ln1_g, lw.ln1_b, T, H, w->ln_eps);
            TT_CHECK_LAUNCH();
        }
        GemmF32Params g1{};
        g1.A = x1; g1.lda = H; g1.W = lw.ffn1_w; g1.bias = lw.ffn1_b; g1.C = ffn; g1.ldc = F; g1.M = T; g1.N = F; g1.K = H;
        if (int rc = gemm_f32(g1, F_EPI_GELU, st)) return rc;
        GemmF32Params g2{};
        g2.A = ffn; g2.lda = F; g2.W = lw.ffn2_w; g2.bias = lw.ffn2_b; g2.residual = x1; g2.ldr = H; g2.C = y; g2.ldc = H;
        g2.M = T; g2.N = H; g2.K = F;
        if (int rc = gemm_f32(g2, F_EPI_RESIDUAL, st)) return rc;
        float* dst = (l == w->layers - 1) ? hidden_out : x;
        {
            TtProfScope prof(TT_K_ROWOPS, st);
            hipLaunchKernelGGL(layernorm_f32_kernel, row_grid_f(T), dim3(kRowThreadsF), 0, st, y, dst, lw.ln2_g, lw.ln2_b, T, H, w->ln_eps);
            TT_CHECK_LAUNCH();
        }
        x = dst;
    }
    return TT_OK;
}

int tt_embed_pool_f32(const float* hidden_f32, int ld, const int32_t* rows, int n_seq, int hidden, float* out_f32,
                      void* out_bf16, void* stream) {
    TT_CHECK_ARG(n_seq >= 0, "n_seq=%d", n_seq);
    if (n_seq == 0) return TT_OK;
    TT_CHECK_ARG(hidden_f32 && rows && out_f32 && ld >= hidden, "bad argument");
    hipStream_t st = (hipStream_t)stream;
    TtProfScope prof(TT_K_ROWOPS, st);
    hipLaunchKernelGGL(cls_pool_f32_kernel, row_grid_f(n_seq), dim3(kRowThreadsF), 0, st, hidden_f32, ld, rows, n_seq, hidden, out_f32,
                       (uint16_t*)out_bf16);
    TT_CHECK_LAUNCH();
    return TT_OK;
}

int tt_rerank_head_f32(const tt_encoder_weights_f32* w, const float* hidden_f32, const int32_t* rows, int n_seq, float* scores,
                       float* logits, void* workspace, size_t workspace_bytes, void* stream) {
    if (int rc = check_weights_f32(w)) return rc;
    TT_CHECK_ARG(w->cls_dense_w && w->cls_dense_b && w->cls_out_w && w->cls_out_b, "weights carry no classification head");
    TT_CHECK_ARG(n_seq >= 0, "n_seq=%d", n_seq);
    if (n_seq == 0) return TT_OK;
    TT_CHECK_ARG(hidden_f32 && rows && scores, "null pointer");
    const int H = w->hidden;
    const int n_pad = (n_seq + 127) / 128 * 128;
    const size_t need = 2 * tt_align_up((size_t)n_pad * H * 4, 256);
    if (!workspace || workspace_bytes < need) {
        tt_set_error("tt_rerank_head_f32: workspace %zu < required %zu bytes", workspace_bytes, need);
        return TT_E_WORKSPACE;
    }
    hipStream_t st = (hipStream_t)stream;
    float* cls = (float*)workspace;
    float* t = (float*)((char*)workspace + tt_align_up((size_t)n_pad * H * 4, 256));
    {
        TtProfScope prof(TT_K_ROWOPS, st);
        hipLaunchKernelGGL(gather_rows_f32_kernel, row_grid_f(n_pad), dim3(kRowThreadsF), 0, st, hidden_f32, H, rows, n_seq, n_pad, H, cls);
        TT_CHECK_LAUNCH();
    }
    GemmF32Params g{};
    g.A = cls; g.lda = H; g.W = w->cls_dense_w; g.bias = w->cls_dense_b; g.C = t; g.ldc = H; g.M = n_pad; g.N = H; g.K = H;
    if (int rc = gemm_f32(g, F_EPI_TANH, st)) return rc;
    TtProfScope prof(TT_K_ROWOPS, st);
    hipLaunchKernelGGL(head_out_f32_kernel, row_grid_f(n_seq), dim3(kRowThreadsF), 0, st, t, H, w->cls_out_w, w->cls_out_b, n_seq, H,
                       scores, logits);
    TT_CHECK_LAUNCH();
    return TT_OK;
}

/* building block for the parity tests: C = epi(A . W^T + bias), fp32; m any, n % 128 == 0, k % 32 == 0 */
int tt_gemm_f32(const float* a, const float* w, const float* bias, const float* residual, float* c, int m, int n, int k,
                int epilogue, void* stream) {
    TT_CHECK_ARG(a && w && bias && c, "null pointer");
    TT_CHECK_ARG(epilogue >= F_EPI_BIAS && epilogue <= F_EPI_TANH, "epilogue %d", epilogue);
    TT_CHECK_ARG(epilogue != F_EPI_RESIDUAL || residual, "residual epilogue without residual");
    GemmF32Params g{};
    g.A = a; g.lda = k; g.W = w; g.bias = bias; g.residual = residual; g.ldr = n; g.C = c; g.ldc = n; g.M = m; g.N = n; g.K = k;
    return gemm_f32(g, epilogue, (hipStream_t)stream);
}

}  // extern "C"
