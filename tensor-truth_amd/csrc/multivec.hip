// BGE-M3's multi-vector head: late interaction at the model's own width (include/tt_hip.h, "Multi-vector head").
//   tt_multivec_project[_f16|_f32]  v = normalize(W h + b) for the listed rows of a hidden state, dim up to 1024, one rounding
//   tt_maxsim_wide[_f16]            scores[q][c] = sum_i max_j <Q_i, D_j> (or its mean over i) for dim up to 1024, queries up to 512
//                                   and documents up to 8192 vectors that already sit in device memory
//   tt_m3_mix                       (w_dense dense + w_lex lex + w_mv mv) / (w_dense + w_lex + w_mv), elementwise
// colbert.hip's kernels hold a query block and all of dim in one wave's registers, which stops at dim 128; these stage the query in
// LDS and spread dim over a workgroup's waves.
//
// The MFMA layout is colbert.hip's (mfma_f32_16x16x32: a lane's operand fragment is 16 contiguous bytes of one row, A rows on
// lane & 15, K offset 8 (lane >> 4); the accumulator of lane l holds rows 4 (l >> 4) + i, i = 0..3, of column l & 15).
//
// Compiled twice like the encoder path (common.h TT_F16): the bf16 object holds everything; the fp16 object the two entries whose
// operands are 16-bit vectors (f16_names.h).
#include "common.h"

#include <algorithm>
#include <cmath>

namespace {

__device__ __forceinline__ float wave_max16(float v) {
    v = fmaxf(v, __shfl_xor(v, 16, 64));
    return fmaxf(v, __shfl_xor(v, 32, 64));
}

// v, or zeros: a select of VALUES (a select between v and a zero constant as objects goes through scratch memory)
__device__ __forceinline__ uint4 keep4(const uint4& v, bool keep) {
    return uint4{keep ? v.x : 0u, keep ? v.y : 0u, keep ? v.z : 0u, keep ? v.w : 0u};
}

constexpr int kMaxDim = 1024, kMaxH = 1024;
constexpr int kWideMaxQuery = 512, kWideMaxDoc = 8192;
constexpr int kWideWaves = 4;                     // waves of a MaxSim workgroup: wave w takes document blocks w, w + 4, ...
constexpr int kWideQTile = 32;                    // query tokens staged in LDS per pass over the document (two MFMA column blocks)
constexpr int kWideChunk = 128;                   // elements of a document row a wave loads per stage: 4 fragments per lane

// ---- MaxSim, dim up to 1024 ---------------------------------------------------------------------------------------------------
// One workgroup per (candidate, query).  A pass stages 32 query tokens in LDS in FRAGMENT order -- fragment (block b, k-step kk) is
// 64 lanes x 16 bytes, lane-contiguous, so a wave's ds_read_b128 of it is conflict-free -- 64 dim bytes (8 KiB at dim 128, 64 KiB at
// 1024).  The document is split across the waves in blocks of 16 rows; a wave streams its blocks from memory once per pass,
// 128 elements of 16 rows (4 KiB) per stage, with the next stage's loads issued before the current stage's MFMAs (two register
// buffers), and multiplies every stage against both query blocks.  Lane l keeps the running maximum of its four document rows of
// query column l & 15 (rows past d_len: -inf).  The maximum is exact and order-free, so splitting a document over waves changes no
// bit: per-wave maxima meet in LDS, and thread 0 adds the q_len maxima in index order in fp32.  Lengths beyond the documented
// limits are clamped, so a bad length array cannot read past a buffer the host sized by those limits.
// One pass of a wave over its document blocks against the staged query tile -> the lane's running maxima for its column of the
// tile's first and (TWO) second block.  Every load is unconditional: a row past the document is clamped to its last row (in bounds:
// d_len >= 1 here) and masked to -inf where the maxima are taken, and the one stage loaded past the wave's last block likewise.
template <bool TWO>
__device__ __forceinline__ void wide_pass(const uint16_t* __restrict__ dbase, int dim, int chunks, int frags, int dl, int my, int wave,
                                          int lane, const uint4* qfrag, float& m0, float& m1) {
    const int c = lane & 15, g = lane >> 4;
    f32x4 s0 = f32x4{0.f, 0.f, 0.f, 0.f}, s1 = s0;
    int cb = 0, cc = 0, pb = 0, pc = 0;   // (block, chunk) of the stage being multiplied / being loaded
    uint4 bufa[4], bufb[4];
#define TT_WIDE_LOAD(buf)                                                                                          \
    {                                                                                                              \
        const int row = min(16 * (wave + kWideWaves * pb) + c, dl - 1);                                            \
        const uint16_t* p = dbase + (size_t)row * dim + pc * kWideChunk;                                           \
        _Pragma("unroll") for (int e = 0; e < 4; ++e) buf[e] = *reinterpret_cast<const uint4*>(p + 32 * e);        \
        if (++pc == chunks) {                                                                                      \
            pc = 0;                                                                                                \
            ++pb;                                                                                                  \
        }                                                                                                          \
    }
#define TT_WIDE_MULTIPLY(buf)                                                                                      \
    {                                                                                                              \
        _Pragma("unroll") for (int e = 0; e < 4; ++e) {                                                            \
            const int kk = 4 * cc + e;                                                                             \
            const ex8 a = __builtin_bit_cast(ex8, buf[e]);                                                         \
            s0 = TT_MFMA_16x16x32(a, __builtin_bit_cast(ex8, qfrag[kk * 64 + lane]), s0);                          \
            if constexpr (TWO) s1 = TT_MFMA_16x16x32(a, __builtin_bit_cast(ex8, qfrag[(frags + kk) * 64 + lane]), s1); \
        }                                                                                                          \
        if (++cc == chunks) { /* the block's dot products are whole */                                             \
            const int r0 = 16 * (wave + kWideWaves * cb) + 4 * g;                                                  \
            _Pragma("unroll") for (int i = 0; i < 4; ++i) {                                                        \
                m0 = fmaxf(m0, r0 + i < dl ? s0[i] : -INFINITY);                                                   \
                if constexpr (TWO) m1 = fmaxf(m1, r0 + i < dl ? s1[i] : -INFINITY);                                \
            }                                                                                                      \
            s0 = f32x4{0.f, 0.f, 0.f, 0.f};                                                                        \
            s1 = s0;                                                                                               \
            cc = 0;                                                                                                \
            ++cb;                                                                                                  \
        }                                                                                                          \
    }
    const int stages = my * chunks;
    if (stages > 0) TT_WIDE_LOAD(bufa)
    for (int it = 0; it < stages; it += 2) {   // (wave-uniform)
        TT_WIDE_LOAD(bufb)
        TT_WIDE_MULTIPLY(bufa)
        if (it + 1 >= stages) break;
        TT_WIDE_LOAD(bufa)
        TT_WIDE_MULTIPLY(bufb)
    }
#undef TT_WIDE_LOAD
#undef TT_WIDE_MULTIPLY
}

__global__ __launch_bounds__(64 * kWideWaves) void maxsim_wide_kernel(const uint16_t* __restrict__ qv, const int32_t* __restrict__ q_start,
                                                                      const int32_t* __restrict__ q_len, const uint16_t* __restrict__ dv,
                                                                      const int64_t* __restrict__ d_start,
                                                                      const int32_t* __restrict__ d_len, const int32_t* __restrict__ cand,
                                                                      int n_cand, int dim, int mean, float* __restrict__ scores) {
    extern __shared__ __attribute__((aligned(16))) char mv_lds[];
    uint4* qfrag = reinterpret_cast<uint4*>(mv_lds);          // [2 blocks][dim / 32 k-steps][64 lanes]
    __shared__ float tok_max[kWideMaxQuery];
    __shared__ float part[kWideWaves][kWideQTile];
    const int ci = blockIdx.x, q = blockIdx.y;
    const int doc = cand ? cand[(size_t)q * n_cand + ci] : ci;
    float* dst = scores + (size_t)q * n_cand + ci;
    if (doc < 0) {   // (workgroup-uniform)
        if (threadIdx.x == 0) *dst = -INFINITY;
        return;
    }
    const int ql = min(max(q_len[q], 0), kWideMaxQuery), dl = min(max(d_len[doc], 0), kWideMaxDoc);
    if (dl == 0 || ql == 0) {
        if (threadIdx.x == 0) *dst = 0.f;
        return;
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, c = lane & 15, g = lane >> 4;
    const int frags = dim >> 5, chunks = dim / kWideChunk;
    const uint16_t* qbase = qv + (size_t)q_start[q] * dim;
    const uint16_t* dbase = dv + (size_t)d_start[doc] * dim + 8 * g;
    const int nblk = (dl + 15) >> 4;
    const int my = nblk > wave ? (nblk - wave + kWideWaves - 1) / kWideWaves : 0;   // document blocks of this wave
    for (int q0 = 0; q0 < ql; q0 += kWideQTile) {   // (workgroup-uniform)
        __syncthreads();   // the previous pass has read its fragments and its per-wave maxima
        for (int idx = threadIdx.x; idx < 2 * frags * 64; idx += 64 * kWideWaves) {
            const int l = idx & 63, f = idx >> 6;
            const int b = f >= frags ? 1 : 0, kk = f - b * frags;
            const int tok = q0 + 16 * b + (l & 15);
            const uint4 v = *reinterpret_cast<const uint4*>(qbase + (size_t)min(tok, ql - 1) * dim + kk * 32 + 8 * (l >> 4));
            qfrag[idx] = keep4(v, tok < ql);
        }
        __syncthreads();
        float m0 = -INFINITY, m1 = -INFINITY;
        if (q0 + 16 < ql)   // (the second column block holds live tokens)
            wide_pass<true>(dbase, dim, chunks, frags, dl, my, wave, lane, qfrag, m0, m1);
        else
            wide_pass<false>(dbase, dim, chunks, frags, dl, my, wave, lane, qfrag, m0, m1);
        m0 = wave_max16(m0);
        m1 = wave_max16(m1);
        if (g == 0) {
            part[wave][c] = m0;
            part[wave][16 + c] = m1;
        }
        __syncthreads();
        if (threadIdx.x < kWideQTile && q0 + (int)threadIdx.x < ql) {
            float m = part[0][threadIdx.x];
#pragma unroll
            for (int w = 1; w < kWideWaves; ++w) m = fmaxf(m, part[w][threadIdx.x]);
            tok_max[q0 + threadIdx.x] = m;
        }
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        float acc = 0.f;
#pragma unroll 8
        for (int i = 0; i < ql; ++i) acc += tok_max[i];
        *dst = mean ? acc / (float)ql : acc;
    }
}

// ---- projection + bias + L2 normalisation of listed rows, dim up to 1024 ----------------------------------------------------------
// One workgroup of eight waves per 64 output rows, so W is read once per 64 rows.  The output rows are the MFMA's columns (B operand:
// 16 bytes of the source row rows[n]; four column blocks), W's rows its rows; wave w owns the 16-wide slices w, w + 8, ... of dim (up
// to 8 of them: 128 accumulator registers).  The bias is added to the fp32 accumulator; the squared norm of a row is summed per lane
// over its slices in ascending order, across the four lane groups, then across the waves through LDS in wave order -- an order that
// depends on dim alone, so a row's bits do not depend on where in a launch it sits.  A source row outside [0, n_rows) gives a zero
// row (no bias).  F32: fp32 hidden states and W on mfma_f32_16x16x4 (a lane's 16 bytes are four k-steps), fp16 out.
constexpr int kProjWaves = 8, kProjBlocks = 4, kProjSlices = kMaxDim / 16 / kProjWaves;

typedef _Float16 mv_h2 __attribute__((ext_vector_type(2)));

template <bool F32>
__device__ __forceinline__ uint32_t pack_out2(float lo, float hi) {
    if constexpr (F32) return __builtin_bit_cast(uint32_t, __builtin_convertvector(f32x2{lo, hi}, mv_h2));   // (|v| <= 1: in range)
    else return pack_e2(lo, hi);
}

template <bool F32>
__device__ __forceinline__ f32x4 project_mma(const uint4& a, const uint4& b, f32x4 acc) {
    if constexpr (F32) {
        const f32x4 af = __builtin_bit_cast(f32x4, a), bf = __builtin_bit_cast(f32x4, b);
#pragma unroll
        for (int e = 0; e < 4; ++e) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(af[e], bf[e], acc, 0, 0, 0);
        return acc;
    } else {
        return TT_MFMA_16x16x32(__builtin_bit_cast(ex8, a), __builtin_bit_cast(ex8, b), acc);
    }
}

template <bool F32>
__global__ __launch_bounds__(64 * kProjWaves) void multivec_project_kernel(const char* __restrict__ hidden, int n_rows, int ld, int H,
                                                                           const char* __restrict__ W, const float* __restrict__ bias,
                                                                           int dim, const int32_t* __restrict__ rows, int n_out,
                                                                           uint16_t* __restrict__ out) {
    constexpr int EL = F32 ? 4 : 8;        // elements of a lane's 16-byte fragment
    constexpr int ES = F32 ? 4 : 2;        // bytes of an element
    constexpr int KS = 4 * EL;             // k advanced per step
    __shared__ float part[kProjWaves][16 * kProjBlocks];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, c = lane & 15, g = lane >> 4;
    const int n0 = blockIdx.x * 16 * kProjBlocks;
    const int nrb = min(kProjBlocks, (n_out - n0 + 15) >> 4);   // column blocks that hold an output row (workgroup-uniform)
    const int slices = dim >> 7;                                // 16-wide slices of dim per wave
    const char* hrow[kProjBlocks];
    bool live[kProjBlocks];
#pragma unroll
    for (int rb = 0; rb < kProjBlocks; ++rb) {
        const int n = n0 + 16 * rb + c;
        const int src = n < n_out ? rows[n] : -1;
        live[rb] = src >= 0 && src < n_rows;
        hrow[rb] = hidden + ((size_t)(live[rb] ? src : 0) * ld + EL * g) * ES;
    }
    f32x4 acc[kProjSlices][kProjBlocks];
#pragma unroll
    for (int j = 0; j < kProjSlices; ++j)
#pragma unroll
        for (int rb = 0; rb < kProjBlocks; ++rb) acc[j][rb] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int k0 = 0; k0 < H; k0 += KS) {
        uint4 hf[kProjBlocks];
#pragma unroll
        for (int rb = 0; rb < kProjBlocks; ++rb)
        {   // (row 0 stands in for a source row that does not exist: the load is in bounds, its value dropped)
            const uint4 v = *reinterpret_cast<const uint4*>(hrow[rb] + (size_t)k0 * ES);
            hf[rb] = keep4(v, live[rb]);
        }
#pragma unroll
        for (int j = 0; j < kProjSlices; ++j) {
            if (j < slices) {   // (workgroup-uniform)
                const int r = 16 * (wave + kProjWaves * j) + c;   // W row of this lane's A fragment (< dim)
                const uint4 wf = *reinterpret_cast<const uint4*>(W + ((size_t)r * H + k0 + EL * g) * ES);
#pragma unroll
                for (int rb = 0; rb < kProjBlocks; ++rb)
                    if (rb < nrb) acc[j][rb] = project_mma<F32>(wf, hf[rb], acc[j][rb]);
            }
        }
    }
    // y = W h + b in fp32 (a zero row for a source row that does not exist), then its squared norm
#pragma unroll
    for (int rb = 0; rb < kProjBlocks; ++rb) {
        float ss = 0.f;
#pragma unroll
        for (int j = 0; j < kProjSlices; ++j) {
            if (j < slices) {
                const float4 b = *reinterpret_cast<const float4*>(bias + 16 * (wave + kProjWaves * j) + 4 * g);
                const float bb[4] = {b.x, b.y, b.z, b.w};
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const float y = live[rb] ? acc[j][rb][i] + bb[i] : 0.f;
                    acc[j][rb][i] = y;
                    ss = fmaf(y, y, ss);
                }
            }
        }
        ss += __shfl_xor(ss, 16, 64);
        ss += __shfl_xor(ss, 32, 64);
        if (g == 0) part[wave][16 * rb + c] = ss;
    }
    __syncthreads();
#pragma unroll
    for (int rb = 0; rb < kProjBlocks; ++rb) {
        const int n = n0 + 16 * rb + c;
        if (n >= n_out) continue;
        float tot = part[0][16 * rb + c];
#pragma unroll
        for (int w = 1; w < kProjWaves; ++w) tot += part[w][16 * rb + c];
        const float den = fmaxf(sqrtf(tot), 1e-12f);
#pragma unroll
        for (int j = 0; j < kProjSlices; ++j) {
            if (j < slices) {
                const int col = 16 * (wave + kProjWaves * j) + 4 * g;
                *reinterpret_cast<uint2*>(out + (size_t)n * dim + col) =
                    uint2{pack_out2<F32>(acc[j][rb][0] / den, acc[j][rb][1] / den), pack_out2<F32>(acc[j][rb][2] / den, acc[j][rb][3] / den)};
            }
        }
    }
}

template <bool F32>
int project_launch(const char* name, const void* hidden, int n_rows, int ld, int H, const void* w, const float* bias, int dim,
                   const int32_t* rows, int n_out, void* out, hipStream_t st) {
    if (H <= 0 || H % 128 || H > kMaxH) {
        tt_set_error("%s: hidden=%d must be a multiple of 128 and <= %d", name, H, kMaxH);
        return TT_E_UNSUPPORTED;
    }
    if (dim <= 0 || dim % 128 || dim > kMaxDim) {
        tt_set_error("%s: dim=%d must be a multiple of 128 and <= %d", name, dim, kMaxDim);
        return TT_E_UNSUPPORTED;
    }
    TT_CHECK_ARG(n_rows > 0 && n_out >= 0 && ld >= H && ld % (F32 ? 4 : 8) == 0, "%s: n_rows=%d n_out=%d ld=%d hidden=%d", name, n_rows,
                 n_out, ld, H);
    if (n_out == 0) return TT_OK;
    TT_CHECK_ARG(hidden && w && bias && rows && out, "%s: null pointer", name);
    TtProfScope prof(TT_K_ROWOPS, st);
    hipLaunchKernelGGL(multivec_project_kernel<F32>, dim3((n_out + 16 * kProjBlocks - 1) / (16 * kProjBlocks)), dim3(64 * kProjWaves), 0,
                       st, (const char*)hidden, n_rows, ld, H, (const char*)w, bias, dim, rows, n_out, (uint16_t*)out);
    TT_CHECK_LAUNCH();
    return TT_OK;
}

#if !TT_F16
// ---- the three-way score -------------------------------------------------------------------------------------------------------
__global__ void m3_mix_kernel(const float* __restrict__ dense, const float* __restrict__ lex, const float* __restrict__ mv, int64_t n,
                              float w_dense, float w_lex, float w_mv, float* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float d = dense[i], l = lex[i], m = mv[i];
    // -inf (a candidate that is none, a removed document) stays -inf whatever its weight: 0 * -inf would be NaN
    out[i] = (d == -INFINITY || l == -INFINITY || m == -INFINITY) ? -INFINITY
                                                                    : (w_dense * d + w_lex * l + w_mv * m) / (w_dense + w_lex + w_mv);
}
#endif

}  // namespace

extern "C" {

int tt_maxsim_wide(const void* q_vecs, const int32_t* q_start, const int32_t* q_len, int n_q, const void* d_vecs, const int64_t* d_start,
                   const int32_t* d_len, const int32_t* cand, int n_cand, int dim, int mean, float* scores, void* stream) {
    const char* name = kF16 ? "tt_maxsim_wide_f16" : "tt_maxsim_wide";
    if (dim <= 0 || dim % 128 || dim > kMaxDim) {
        tt_set_error("%s: dim=%d must be a multiple of 128 and <= %d", name, dim, kMaxDim);
        return TT_E_UNSUPPORTED;
    }
    TT_CHECK_ARG(n_q >= 0 && n_cand >= 0 && n_q <= 65535, "%s: n_q=%d n_cand=%d", name, n_q, n_cand);
    if (n_q == 0 || n_cand == 0) return TT_OK;
    TT_CHECK_ARG(q_vecs && q_start && q_len && d_vecs && d_start && d_len && scores, "%s: null pointer", name);
    hipStream_t st = (hipStream_t)stream;
    const size_t lds = (size_t)kWideQTile * dim * sizeof(uint16_t);
    TT_SET_MAX_LDS(maxsim_wide_kernel, (size_t)kWideQTile * kMaxDim * sizeof(uint16_t));
    TtProfScope prof(TT_K_ROWOPS, st);
    hipLaunchKernelGGL(maxsim_wide_kernel, dim3(n_cand, n_q), dim3(64 * kWideWaves), lds, st, (const uint16_t*)q_vecs, q_start, q_len,
                       (const uint16_t*)d_vecs, d_start, d_len, cand, n_cand, dim, mean, scores);
    TT_CHECK_LAUNCH();
    return TT_OK;
}

int tt_multivec_project(const void* hidden, int n_rows, int ld, int H, const void* w, const float* bias, int dim, const int32_t* rows,
                        int n_out, void* out, void* stream) {
    return project_launch<false>(kF16 ? "tt_multivec_project_f16" : "tt_multivec_project", hidden, n_rows, ld, H, w, bias, dim, rows,
                                 n_out, out, (hipStream_t)stream);
}

#if !TT_F16
int tt_multivec_project_f32(const float* hidden, int n_rows, int ld, int H, const float* w, const float* bias, int dim,
                            const int32_t* rows, int n_out, void* out, void* stream) {
    return project_launch<true>("tt_multivec_project_f32", hidden, n_rows, ld, H, w, bias, dim, rows, n_out, out, (hipStream_t)stream);
}

int tt_m3_mix(const float* dense, const float* lex, const float* mv, int64_t n, float w_dense, float w_lex, float w_mv, float* out,
              void* stream) {
    TT_CHECK_ARG(n >= 0, "tt_m3_mix: n=%lld", (long long)n);
    const float sum = w_dense + w_lex + w_mv;
    TT_CHECK_ARG(w_dense >= 0.f && w_lex >= 0.f && w_mv >= 0.f && sum > 0.f && std::isfinite(sum),
                 "tt_m3_mix: w_dense=%g w_lex=%g w_mv=%g (all >= 0, finite, not all 0)", (double)w_dense, (double)w_lex, (double)w_mv);
    if (n == 0) return TT_OK;
    TT_CHECK_ARG(dense && lex && mv && out, "tt_m3_mix: null pointer");
    hipStream_t st = (hipStream_t)stream;
    TtProfScope prof(TT_K_ROWOPS, st);
    hipLaunchKernelGGL(m3_mix_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, dense, lex, mv, n, w_dense, w_lex, w_mv, out);
    TT_CHECK_LAUNCH();
    return TT_OK;
}
#endif

}  // extern "C"
