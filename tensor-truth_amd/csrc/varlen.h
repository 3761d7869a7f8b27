// What the packed-varlen model families share (decoder.hip: Qwen3; modernbert.hip: ModernBERT; t5.hip; gemma.hip; and, for the
// attention tile and the argument checks, mpnet.hip: MPNet's post-LN layer with a relative-position bias, and deberta.hip:
// DeBERTa-v2/v3's post-LN layer with disentangled attention; jinabert.hip: JinaBERT's post-LN layer with ALiBi): the attention
// tile over the V8 layout and its windowed wrapper, the embedding gather, RMSNorm, the gated activation and its gates, the workspace
// plan and the shape and argument checks.  The pre-norm families' shared block is prenorm.h, the post-LN families' postln.h, the
// sentence-transformers tail (its pooling loop is here) pool_dense.h -- all on top of this header.
// Device code sits in an anonymous namespace or is a template: one copy per translation unit and element type (common.h TT_F16).
#pragma once
#include "common.h"
#include "encoder.h"

#include <algorithm>

namespace {

__device__ __forceinline__ float wave_max16(float v) {
    // maximum over the four lanes l, l ^ 16, l ^ 32, l ^ 48 (one query column of an MFMA 16x16 result)
    v = fmaxf(v, __shfl_xor(v, 16, 64));
    return fmaxf(v, __shfl_xor(v, 32, 64));
}

// ---- embedding gather: out[r] = table[ids[r]] (an id outside [0, vocab) gives a zero row); launched with 128 threads ---------
__global__ __launch_bounds__(128) void embed_gather_kernel(const int32_t* __restrict__ ids, const uint16_t* __restrict__ table,
                                                           int vocab, int H, uint16_t* __restrict__ out) {
    const int row = blockIdx.x;
    const int id = ids[row];
    const bool ok = id >= 0 && id < vocab;
    const uint4* src = reinterpret_cast<const uint4*>(table + (size_t)(ok ? id : 0) * H);
    uint4* dst = reinterpret_cast<uint4*>(out + (size_t)row * H);
    for (int c = threadIdx.x; c < H / 8; c += blockDim.x) dst[c] = ok ? src[c] : uint4{0u, 0u, 0u, 0u};
}

inline int embed_gather_launch(const int32_t* ids, const void* table, int vocab, int H, uint16_t* out, int rows, hipStream_t st) {
    TtProfScope prof(TT_K_ROWOPS, st);
    hipLaunchKernelGGL(embed_gather_kernel, dim3(rows), dim3(128), 0, st, ids, (const uint16_t*)table, vocab, H, out);
    TT_CHECK_LAUNCH();
    return TT_OK;
}

// ---- RMSNorm over rows of H <= 1024 elements: one wave per row, four rows per block ---------------------------------------------
// fp32 statistics.  ROUND_BEFORE_WEIGHT = false (Qwen3): out = e(v * rsqrt(mean(v^2) + eps) * w), one rounding to the element type.
// ROUND_BEFORE_WEIGHT = true (T5LayerNorm): out = e(e(v * rsqrt(mean(v^2) + eps)) * w), the normalised value rounded to the
// element type BEFORE the weight multiplies it, as transformers' T5LayerNorm does with 16-bit weights; the second product is exact
// in fp32 when w holds values of the element type.
template <bool ROUND_BEFORE_WEIGHT>
__global__ __launch_bounds__(256) void rmsnorm_kernel(const uint16_t* __restrict__ in, uint16_t* __restrict__ out,
                                                      const float* __restrict__ g, int rows, int H, float eps) {
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    const uint4* src = reinterpret_cast<const uint4*>(in + (size_t)row * H);
    uint4* dst = reinterpret_cast<uint4*>(out + (size_t)row * H);
    const int nc = H / 8;   // <= 128 chunks of 8 elements: at most two per lane
    uint4 v[2];
    float ss = 0.f;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int c = lane + 64 * j;
        v[j] = c < nc ? src[c] : uint4{0u, 0u, 0u, 0u};
        const uint32_t u[4] = {v[j].x, v[j].y, v[j].z, v[j].w};
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const float a = elo(u[k]), b = ehi(u[k]);
            ss += a * a;
            ss += b * b;
        }
    }
    const float r = rsqrtf(wave_sum(ss) / (float)H + eps);
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int c = lane + 64 * j;
        if (c >= nc) continue;
        const uint32_t u[4] = {v[j].x, v[j].y, v[j].z, v[j].w};
        uint32_t o[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int e = 8 * c + 2 * k;
            if constexpr (ROUND_BEFORE_WEIGHT) {
                const uint32_t n2 = pack_e2(elo(u[k]) * r, ehi(u[k]) * r);   // the first rounding
                o[k] = pack_e2(elo(n2) * g[e], ehi(n2) * g[e + 1]);
            } else {
                o[k] = pack_e2(elo(u[k]) * r * g[e], ehi(u[k]) * r * g[e + 1]);
            }
        }
        dst[c] = uint4{o[0], o[1], o[2], o[3]};
    }
}

template <bool ROUND_BEFORE_WEIGHT>
int rmsnorm_launch(const uint16_t* in, uint16_t* out, const float* g, int rows, int H, float eps, hipStream_t st) {
    TtProfScope prof(TT_K_ROWOPS, st);
    hipLaunchKernelGGL(rmsnorm_kernel<ROUND_BEFORE_WEIGHT>, dim3((rows + 3) / 4), dim3(256), 0, st, in, out, g, rows, H, eps);
    TT_CHECK_LAUNCH();
    return TT_OK;
}

// ---- gated activation: gu [T][2F] (activated columns, then the columns that multiply them) -> out [T][F] ---------------------
// out = Act::f(gu[:, :F]) * gu[:, F:], Act::f one fp32 value at a time (GeluErf, Silu and GeluTanh below)
template <class Act>
__global__ __launch_bounds__(256) void gated_act_kernel(const uint16_t* __restrict__ gu, uint16_t* __restrict__ out, int64_t n_chunks,
                                                        int F) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_chunks) return;
    const int64_t row = i / (F / 8), c = i % (F / 8);
    const uint4 av = reinterpret_cast<const uint4*>(gu + row * 2 * F)[c];
    const uint4 mv = reinterpret_cast<const uint4*>(gu + row * 2 * F + F)[c];
    const uint32_t a4[4] = {av.x, av.y, av.z, av.w}, m4[4] = {mv.x, mv.y, mv.z, mv.w};
    uint32_t o[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) o[k] = pack_e2(Act::f(elo(a4[k])) * elo(m4[k]), Act::f(ehi(a4[k])) * ehi(m4[k]));
    reinterpret_cast<uint4*>(out + row * F)[c] = uint4{o[0], o[1], o[2], o[3]};
}

template <class Act>
int gated_act_launch(const uint16_t* gu, uint16_t* out, int rows, int F, hipStream_t st) {
    TtProfScope prof(TT_K_ROWOPS, st);
    const int64_t chunks = (int64_t)rows * (F / 8);
    hipLaunchKernelGGL(gated_act_kernel<Act>, dim3((unsigned)((chunks + 255) / 256)), dim3(256), 0, st, gu, out, chunks, F);
    TT_CHECK_LAUNCH();
    return TT_OK;
}

// GELU(x) = 0.5 x (1 + erf(x / sqrt 2)), the exact-erf form of the encoder's GEMM epilogue (gemm.hip gelu_erf2, one value at a
// time): gelu(x) = max(x, 0) - |x| 2^Q(|x|), Q the degree-7 fit of log2 Phi(-u) on [0, 9]; abs error <= 1e-5.
__device__ __forceinline__ float mb_gelu_erf(float x) {
    const float u = fabsf(x);
    float q = u * -9.697845371e-07f + 4.016999810e-05f;
    q = q * u + -7.211678312e-04f;
    q = q * u + 7.490924560e-03f;
    q = q * u + -5.142170191e-02f;
    q = q * u + -4.614778757e-01f;
    q = q * u + -1.149914980e+00f;
    q = q * u + -1.000091195e+00f;
    return fmaxf(x, 0.f) - u * __builtin_amdgcn_exp2f(q);
}
// GELU_erf(input) * gate through varlen.h's gated_act_kernel: gu [T][2F] (input columns, then gate columns) -> out [T][F]
struct GeluErf {
    static __device__ __forceinline__ float f(float x) { return mb_gelu_erf(x); }
};
// SiLU(gate) * up through gated_act_kernel: gu [T][2F] (gate columns, then up columns) -> out [T][F]
struct Silu {
    static __device__ __forceinline__ float f(float x) { return x / (1.0f + expf(-x)); }
};
// GELU_tanh(gate) * up (EmbeddingGemma; T5 v1.1's gelu_new, transformers NewGELUActivation, is the same function):
// 0.5 x (1 + tanh(u)), u = sqrt(2 / pi) (x + 0.044715 x^3), written as x / (1 + exp(-2 u)) (1 + tanh(u) = 2 / (1 + exp(-2 u))), fp32
struct GeluTanh {
    static __device__ __forceinline__ float f(float x) {
        const float u = 0.7978845608028654f * (x + 0.044715f * x * x * x);
        return x / (1.0f + expf(-2.0f * u));
    }
};

// ---- the sum of the rows s0 .. s0 + n - 1 of `hidden` [.][ld], one wave: lane owns the 8-element chunks lane, lane + 64 (H <= 1024)
// (the mean pooling of pool_dense.h's tail and of modernbert.hip's classification head)
// A column is summed in ascending row order, 16-byte reads (any row may start a range).  s0 < 0 or n <= 0: zeros.
__device__ __forceinline__ void pool_rows_sum(const uint16_t* __restrict__ hidden, int ld, int s0, int n, int H, int lane,
                                              float (&acc)[2][8]) {
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int k = 0; k < 8; ++k) acc[j][k] = 0.f;
    if (s0 >= 0) {
        for (int r = 0; r < n; ++r) {
            const uint4* src = reinterpret_cast<const uint4*>(hidden + (size_t)(s0 + r) * ld);
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                const int ch = lane + 64 * j;
                if (ch >= H / 8) continue;
                const uint4 v = src[ch];
                const uint32_t u[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    acc[j][2 * k] += elo(u[k]);
                    acc[j][2 * k + 1] += ehi(u[k]);
                }
            }
        }
    }
}

// ---- embeddings: out[r] = LayerNorm(word[ids[r]] + type[0]) * gamma + beta ------------------------------------------------------
// One wave per row, four rows per block, as rowops.hip: lane l holds the 16-byte pieces l and l + 64 of the row (H <= 1024), the sum
// in fp32, two-pass statistics (mean, then centred variance), one rounding.  An id outside [0, vocab) is clamped into the table
// (the host validates too).
constexpr int kRbRowThreads = 256;

__device__ __forceinline__ void rb_unpack8(const uint4& u, float (&f)[8]) {
    f[0] = elo(u.x); f[1] = ehi(u.x);
    f[2] = elo(u.y); f[3] = ehi(u.y);
    f[4] = elo(u.z); f[5] = ehi(u.z);
    f[6] = elo(u.w); f[7] = ehi(u.w);
}

__global__ __launch_bounds__(kRbRowThreads) void rb_embed_ln_kernel(const int32_t* __restrict__ ids, const uint16_t* __restrict__ word,
                                                                    const uint16_t* __restrict__ type_row, const float* __restrict__ gamma,
                                                                    const float* __restrict__ beta, uint16_t* __restrict__ out, int T,
                                                                    int H, int vocab, float eps) {
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * (kRbRowThreads / 64) + (threadIdx.x >> 6);
    if (row >= T) return;   // (wave-uniform)
    int id = ids[row];
    id = id < 0 ? 0 : (id >= vocab ? vocab - 1 : id);
    const int nch = H / 8;
    float x[2][8];
    float s = 0.f;
#pragma unroll
    for (int c = 0; c < 2; ++c) {
        const int ch = lane + 64 * c;
        if (ch < nch) {
            float a[8], t[8];
            rb_unpack8(*reinterpret_cast<const uint4*>(word + (size_t)id * H + ch * 8), a);
            rb_unpack8(*reinterpret_cast<const uint4*>(type_row + ch * 8), t);
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                x[c][i] = a[i] + t[i];
                s += x[c][i];
            }
        }
    }
    const float mean = wave_sum(s) / (float)H;
    float v = 0.f;
#pragma unroll
    for (int c = 0; c < 2; ++c)
        if (lane + 64 * c < nch)
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                const float d = x[c][i] - mean;
                v += d * d;
            }
    const float rstd = rsqrtf(wave_sum(v) / (float)H + eps);
#pragma unroll
    for (int c = 0; c < 2; ++c) {
        const int ch = lane + 64 * c;
        if (ch < nch) {
            const float4 g0 = *reinterpret_cast<const float4*>(gamma + ch * 8);
            const float4 g1 = *reinterpret_cast<const float4*>(gamma + ch * 8 + 4);
            const float4 b0 = *reinterpret_cast<const float4*>(beta + ch * 8);
            const float4 b1 = *reinterpret_cast<const float4*>(beta + ch * 8 + 4);
            const float g[8] = {g0.x, g0.y, g0.z, g0.w, g1.x, g1.y, g1.z, g1.w};
            const float b[8] = {b0.x, b0.y, b0.z, b0.w, b1.x, b1.y, b1.z, b1.w};
            float y[8];
#pragma unroll
            for (int i = 0; i < 8; ++i) y[i] = (x[c][i] - mean) * rstd * g[i] + b[i];
            *reinterpret_cast<uint4*>(out + (size_t)row * H + ch * 8) =
                uint4{pack_e2(y[0], y[1]), pack_e2(y[2], y[3]), pack_e2(y[4], y[5]), pack_e2(y[6], y[7])};
        }
    }
}

// ---- attention over packed varlen sequences: one 16-query tile of one (sequence b, query head h) per call, one wave -------------
// Query head h reads KV head h / group (group = 1: as many KV heads as query heads).  Tile t holds the queries q0 .. q0 + 15,
// q0 = s0 + 16 t, of the sequence s0 .. s_end - 1.  Keys are visited in blocks of 32 on the absolute 8-row grid (the Alibi policy:
// counted from s0, see below):
//   WINDOW = false (causal):        the blocks from the sequence's first 8-row group up to the tile's last query; key k is live for
//                                   query q iff s0 <= k <= q;
//   WINDOW = true (bidirectional):  the blocks that intersect [max(s0, q0 - w), min(s_end - 1, q0 + 15 + w)]; key k is live for query
//                                   q iff s0 <= k < s_end && |q - k| <= w.  w >= the batch's longest sequence: every key of the
//                                   sequence, the walk and the bits of attention without a window.  (The callers keep w <= n_rows:
//                                   q + w does not overflow.)
// Either mask also removes the neighbouring sequences' rows of shared 8-row groups.
//   S^T = K Q^T  (mfma 16x16x32, two tiles per key block).  The K rows each lane loads are permuted so that, for query c = lane & 15,
//                lane l ends up holding the scores of keys kb + 8 (l >> 4) + j, j = 0..7 -- exactly the B operand of
//   O^T += V^T P^T  (mfma 16x16x32 per 16 features), whose A operand is one 16-byte read of the V8 layout per lane.
// Softmax in fp32 with a running maximum (log2 domain), P rounded to the element type for the product; the denominator sums the
// rounded P, so the weights of a row sum to one as they are applied.  A block may hold no live key for some query of the tile (past
// a window's edge, or past an earlier query of a causal tile): its P is zero and its running maximum stays where it was (-1e30
// before the query's first live key, which only a window can put behind the tile's first block).  Each result column, maximum and
// denominator belongs to one query: what a query gets does not depend on what the other 15 of its tile may see.
// The kernels walk the sequences (a grid's y extent stops at 65535) and decode (b, h, t) from their own grids.
// keep_row < 0: every query of the tile is stored, at its own row of `out`.  keep_row >= 0 (a pooled-row tail): only the query
// at absolute row keep_row is stored, at row out_row of `out` -- the same arithmetic, so the same bits as the full tile gives it.
// Bias policy (MPNet's relative-position bias, mpnet.hip): what is added to a score, in log2 units, before the mask.
//   NoBias (default): nothing -- the code of a tile without the parameter.
//   RelBias: x = s * scale_log2 + tbl[clamp(key - query, -R, R) + R], tbl the head's 2R + 1 floats.  The workgroup stages them in
//            LDS once, PAD copies of the end values on either side (relbias_stage): a lane's eight keys of a block are eight
//            consecutive distances, so ONE clamp of the first distance to [-R - PAD, R + 1] leaves eight consecutive reads that
//            give the clamped entries (all eight at tbl[0] below the range, all at tbl[2R] above it).  Dword reads: within a
//            32-lane half the first distances 8 g - c span 24 consecutive dwords -- distinct banks, equal addresses broadcast.
//   Disentangled (DeBERTa-v2/v3, deberta.hip): x = (s + C[query][i] + P[key][i]) * scale_log2, i = idx[query - key]: the two
//            position terms of a live (query, key) pair, read from the fp32 score tables a launch before the attention wrote
//            (C[t][h][w] = Q[t,h] . PK[w,h], P[t][h][w] = K[t,h] . PQ[w,h]) and added to the RAW score.  The workgroup stages the
//            index table (distance d at d + center) in LDS once, PAD copies of the end values on either side (disent_stage): a
//            lane's eight keys of a block are eight consecutive distances, descending, so one clamp of the first leaves eight
//            reads that are exact wherever the distance is one a sequence can hold.  Masked pairs read nothing.
//   Alibi (JinaBERT, jinabert.hip): x = s * scale_log2 - slope_log2 * float(|key - query|), slope_log2 the head's ALiBi slope times
//            log2(e), rounded once from double by the host.  Computed in registers from the row numbers: no table, no LDS, no
//            clamp -- a distance within a packed batch is below 2^24 and converts exactly, so the bias is exact to its two
//            roundings (the product, the subtraction; one if the compiler contracts them) at any distance.
//            The policy is also ANCHORED: its key blocks are counted from the sequence's own first row, kb = s0 (mod 8), not from
//            the batch's 8-row grid, so a sequence's rows are the same bits wherever it starts -- on the grid (what pack_tokens
//            gives) or right behind its neighbour.  K rows are read row by row either way; a lane's eight V values of a block
//            then straddle two 8-row groups of the V8 layout when s0 is off the grid: two 16-byte reads and a funnel shift by
//            s0 % 8 elements (v8_shift; wave-uniform, and a start on the grid takes the one read of every other policy).
struct NoBias {
    static constexpr bool on = false, content = false, linear = false, anchored = false;
};
struct RelBias {
    static constexpr bool on = true, content = false, linear = false, anchored = false;
    static constexpr int R = 128, PAD = 8, LDS_FLOATS = 2 * R + 1 + 2 * PAD;
    const float* lds;   // the staged table: lds[i] = tbl[clamp(i - PAD, 0, 2R)]
};
// stage head h's table (tbl + h * (2R + 1)) for RelBias; every thread of the workgroup calls it, `lds` holds LDS_FLOATS floats
__device__ __forceinline__ void relbias_stage(const float* __restrict__ tbl, int h, float* lds) {
    for (int i = threadIdx.x; i < RelBias::LDS_FLOATS; i += blockDim.x)
        lds[i] = tbl[(size_t)h * (2 * RelBias::R + 1) + min(max(i - RelBias::PAD, 0), 2 * RelBias::R)];
    __syncthreads();
}

struct Disentangled {
    static constexpr bool on = false, content = true, linear = false, anchored = false;
    static constexpr int PAD = 8, MAX_POS = 512, LDS_INTS = 2 * MAX_POS - 1 + 2 * PAD;
    const int32_t* idx;   // the staged index table: idx[i] = clamp(dist_index[clamp(i - PAD, 0, 2 max_pos - 2)], 0, n_pos - 1)
    int center, idx_max;  // max_pos - 1, 2 max_pos - 2
    const float* c;       // the head's column block of C: C + h * n_pos, rows of ld floats
    const float* p;       // likewise of P
    size_t ld;            // heads * n_pos
};
// stage the index table for Disentangled; every thread of the workgroup calls it, `lds` holds LDS_INTS ints (max_pos <= MAX_POS)
__device__ __forceinline__ void disent_stage(const int32_t* __restrict__ dist_index, int max_pos, int n_pos, int32_t* lds) {
    const int n = 2 * max_pos - 1;
    for (int i = threadIdx.x; i < n + 2 * Disentangled::PAD; i += blockDim.x)
        lds[i] = min(max(dist_index[min(max(i - Disentangled::PAD, 0), n - 1)], 0), n_pos - 1);
    __syncthreads();
}

// ALiBi (JinaBERT, jinabert.hip): the head's slope times log2(e), one register; nothing is staged and nothing is clamped
// the 16-bit elements r .. r + 7 of the sixteen in (a, b), r in 1 .. 7 and wave-uniform: eight consecutive rows of one feature that
// start r rows into an 8-row group of the V8 layout
__device__ __forceinline__ uint4 v8_shift(const uint4& a, const uint4& b, int r) {
    const uint32_t d[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
    uint32_t e[5];
    switch (r >> 1) {
        case 0: e[0] = d[0]; e[1] = d[1]; e[2] = d[2]; e[3] = d[3]; e[4] = d[4]; break;
        case 1: e[0] = d[1]; e[1] = d[2]; e[2] = d[3]; e[3] = d[4]; e[4] = d[5]; break;
        case 2: e[0] = d[2]; e[1] = d[3]; e[2] = d[4]; e[3] = d[5]; e[4] = d[6]; break;
        default: e[0] = d[3]; e[1] = d[4]; e[2] = d[5]; e[3] = d[6]; e[4] = d[7]; break;
    }
    if (r & 1)
        return uint4{(e[0] >> 16) | (e[1] << 16), (e[1] >> 16) | (e[2] << 16), (e[2] >> 16) | (e[3] << 16), (e[3] >> 16) | (e[4] << 16)};
    return uint4{e[0], e[1], e[2], e[3]};
}
struct Alibi {
    static constexpr bool on = false, content = false, linear = true, anchored = true;
    float slope_log2;
};

template <int D, bool WINDOW, class Bias = NoBias>
__device__ __forceinline__ void attention_tile(const uint16_t* __restrict__ qkv, int ld, int q_col0, int k_col0,
                                               const uint16_t* __restrict__ vt, int ldvt, uint16_t* __restrict__ out, int ld_out,
                                               const int32_t* __restrict__ seq_start, const int32_t* __restrict__ seq_len, int n_rows,
                                               int group, int w, float scale_log2, int b, int h, int t, int keep_row = -1,
                                               int out_row = 0, Bias bias = Bias{}) {
    const int s0 = seq_start[b], L = seq_len[b];
    if (s0 < 0 || 16 * t >= L) return;
    const int s_end = min(s0 + L, n_rows);
    const int q0 = s0 + 16 * t;
    if (q0 >= s_end) return;
    const int lane = threadIdx.x, c = lane & 15, g = lane >> 4;
    const int kvh = h / group;
    const uint4 zero4 = uint4{0u, 0u, 0u, 0u};

    // Q fragment, the B operand of S^T: lane holds Q[q0 + c][32 kk + 8 g + j]
    ex8 qf[D / 32];
    const int qrow = q0 + c;
    const int q_lim = min(qrow, s_end - 1);      // rows past the sequence: computed against its keys, never stored
#pragma unroll
    for (int kk = 0; kk < D / 32; ++kk) {
        const uint4 u = qrow < s_end ? *reinterpret_cast<const uint4*>(qkv + (size_t)qrow * ld + q_col0 + h * D + kk * 32 + 8 * g)
                                     : zero4;
        qf[kk] = __builtin_bit_cast(ex8, u);
    }
    f32x4 o[D / 16];
#pragma unroll
    for (int dt = 0; dt < D / 16; ++dt) o[dt] = f32x4{0.f, 0.f, 0.f, 0.f};
    float m = -1e30f, l = 0.f;   // running maximum (log2 units) of query c, and this lane's share of the denominator

    const int q_last = min(q0 + 15, s_end - 1);
    const int k_first = WINDOW ? max(s0, q0 - w) : s0, k_last = WINDOW ? min(s_end - 1, q_last + w) : q_last;   // the tile's keys
    const int k_lo = WINDOW ? max(s0, q_lim - w) : s0, k_hi = WINDOW ? min(s_end - 1, q_lim + w) : q_lim;       // this lane's query's
    const uint16_t* kbase = qkv + k_col0 + (size_t)kvh * D + 8 * g;
    const uint16_t* vbase = vt + ((size_t)kvh * D + c) * 8;
    // the first key block: on the batch's 8-row grid, or (an anchored policy) a multiple of 8 rows behind the sequence's first row
    const int kb0 = Bias::anchored ? k_first - ((k_first - s0) & 7) : k_first & ~7;
    for (int kb = kb0; kb <= k_last; kb += 32) {
        f32x4 s[2];
#pragma unroll
        for (int tt = 0; tt < 2; ++tt) {
            // A row c of tile tt is key kb + 8 (c >> 2) + 4 tt + (c & 3): result row 4 g + i is then key kb + 8 g + 4 tt + i
            const int krow = kb + 8 * (c >> 2) + 4 * tt + (c & 3);
            s[tt] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int kk = 0; kk < D / 32; ++kk) {
                const uint4 u = krow < n_rows ? *reinterpret_cast<const uint4*>(kbase + (size_t)krow * ld + kk * 32) : zero4;
                s[tt] = TT_MFMA_16x16x32(__builtin_bit_cast(ex8, u), qf[kk], s[tt]);
            }
        }
        float x[8];
        float bm = -INFINITY;
        const float* brow = nullptr;   // RelBias: the staged entry of this lane's first key of the block
        if constexpr (Bias::on)
            brow = bias.lds + (min(max(kb + 8 * g - qrow, -Bias::R - Bias::PAD), Bias::R + 1) + Bias::R + Bias::PAD);
        const int32_t* irow = nullptr;  // Disentangled: the staged index of this lane's first key of the block (the next keys': irow[-j])
        const float* crow = nullptr;    //               and the C row of this lane's query
        if constexpr (Bias::content) {
            irow = bias.idx + (min(max(q_lim - (kb + 8 * g) + bias.center, -1), bias.idx_max + Bias::PAD) + Bias::PAD);
            crow = bias.c + (size_t)q_lim * bias.ld;
        }
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int key = kb + 8 * g + j;
            float v;
            if constexpr (Bias::content) {
                float sv = s[j >> 2][j & 3];
                if (key >= k_lo && key <= k_hi) {   // (a live key is a row of the batch and within max_pos of the query)
                    const int i = irow[-j];
                    sv += crow[i] + bias.p[(size_t)key * bias.ld + i];
                }
                v = sv * scale_log2;
            } else if constexpr (Bias::linear) {
                v = s[j >> 2][j & 3] * scale_log2 - bias.slope_log2 * (float)abs(key - qrow);
            } else {
                v = s[j >> 2][j & 3] * scale_log2;
            }
            if constexpr (Bias::on) v += brow[j];
            x[j] = (key >= k_lo && key <= k_hi) ? v : -INFINITY;
            bm = fmaxf(bm, x[j]);
        }
        const float m_new = fmaxf(m, wave_max16(bm));
        const float alpha = exp2f(m - m_new);
        m = m_new;
        uint32_t pk[4];
        float ps = 0.f;
#pragma unroll
        for (int j = 0; j < 8; j += 2) {
            pk[j >> 1] = pack_e2_inrange(exp2f(x[j] - m_new), exp2f(x[j + 1] - m_new));
            ps += elo(pk[j >> 1]);
            ps += ehi(pk[j >> 1]);
        }
        l = l * alpha + ps;
        const ex8 pf = __builtin_bit_cast(ex8, uint4{pk[0], pk[1], pk[2], pk[3]});
        // V^T fragment: feature 16 dt + c, keys kb + 8 g .. + 7 (one 8-row group of the V8 layout)
        const int grp = (kb >> 3) + g;
        const bool vok = 8 * grp < n_rows;
        if constexpr (Bias::anchored) {
            if (s0 & 7) {   // (wave-uniform) keys kb + 8 g .. + 7 start s0 % 8 rows into group grp
                const bool vok1 = 8 * (grp + 1) < n_rows;
#pragma unroll
                for (int dt = 0; dt < D / 16; ++dt) {
                    const uint16_t* vp = vbase + (size_t)grp * ldvt + (size_t)dt * 16 * 8;
                    const uint4 u0 = vok ? *reinterpret_cast<const uint4*>(vp) : zero4;
                    const uint4 u1 = vok1 ? *reinterpret_cast<const uint4*>(vp + ldvt) : zero4;
                    o[dt] = TT_MFMA_16x16x32(__builtin_bit_cast(ex8, v8_shift(u0, u1, s0 & 7)), pf, o[dt] * alpha);
                }
                continue;
            }
        }
#pragma unroll
        for (int dt = 0; dt < D / 16; ++dt) {
            const uint4 u = vok ? *reinterpret_cast<const uint4*>(vbase + (size_t)grp * ldvt + (size_t)dt * 16 * 8) : zero4;
            o[dt] = TT_MFMA_16x16x32(__builtin_bit_cast(ex8, u), pf, o[dt] * alpha);
        }
    }
    l += __shfl_xor(l, 16, 64);
    l += __shfl_xor(l, 32, 64);
    if (qrow < s_end && (keep_row < 0 || qrow == keep_row)) {   // (the only lane-dependent branch: the wave is whole again for the next sequence's tile)
        const float inv = 1.0f / l;
        uint16_t* dst = out + (size_t)(keep_row < 0 ? qrow : out_row) * ld_out + h * D + 4 * g;
#pragma unroll
        for (int dt = 0; dt < D / 16; ++dt)
            *reinterpret_cast<uint2*>(dst + dt * 16) = uint2{pack_e2(o[dt][0] * inv, o[dt][1] * inv),
                                                             pack_e2(o[dt][2] * inv, o[dt][3] * inv)};
    }
}

// ---- bidirectional GQA attention with a sliding window over packed varlen sequences (ModernBERT: D = 64, group 1; EmbeddingGemma:
// D = 256): one wave per (16-query tile, sequence, query head) on the tile above with the window mask
template <int D>
__global__ __launch_bounds__(64) void window_attention_kernel(const uint16_t* __restrict__ qkv, int ld, int q_col0, int k_col0,
                                                              const uint16_t* __restrict__ vt, int ldvt, uint16_t* __restrict__ out,
                                                              int ld_out, const int32_t* __restrict__ seq_start,
                                                              const int32_t* __restrict__ seq_len, int n_seq, int n_rows, int group,
                                                              int w, float scale_log2) {
    const int t = blockIdx.x;
    for (int b = blockIdx.y; b < n_seq; b += gridDim.y)   // (wave-uniform: every lane takes the same sequences)
        attention_tile<D, true>(qkv, ld, q_col0, k_col0, vt, ldvt, out, ld_out, seq_start, seq_len, n_rows, group, w, scale_log2, b,
                                blockIdx.z, t);
}

// window < 0: no window
template <int D>
int window_attention_launch(const uint16_t* qkv, int ld, int q_col0, int k_col0, const uint16_t* vt, int ldvt, uint16_t* out, int ld_out,
                            const int32_t* seq_start, const int32_t* seq_len, int n_seq, int n_rows, int heads, int kv_heads, int max_len,
                            int window, hipStream_t st) {
    static_assert(D == 64 || D == 256, "head widths with a window: 64, 256");
    const int n_qt = (max_len + 15) / 16;
    const dim3 grid(n_qt, std::min(n_seq, 65535), heads);   // more sequences: each block row takes every 65535th
    const float scale_log2 = 1.4426950408889634f / (D == 64 ? 8.0f : 16.0f);   // log2(e) / sqrt(D)
    const int w = (window < 0 || window > n_rows) ? n_rows : window;   // |q - k| < n_rows within a batch
    TtProfScope prof(TT_K_ATTENTION, st);
    hipLaunchKernelGGL(window_attention_kernel<D>, grid, dim3(64), 0, st, qkv, ld, q_col0, k_col0, vt, ldvt, out, ld_out, seq_start,
                       seq_len, n_seq, n_rows, heads / kv_heads, w, scale_log2);
    TT_CHECK_LAUNCH();
    return TT_OK;
}

// ---- host side -------------------------------------------------------------------------------------------------------------------
// One forward's workspace: the residual stream twice (ha, hb), the normed rows x, the projections' outputs and the fp32 zeros that
// stand in for the biases (and LayerNorm betas) these models do not have.  Rows are padded to the 256-row GEMM tile.
struct VarlenWs {
    size_t off_ha, off_hb, off_x, off_qkv, off_vt, off_ctx, off_gu, off_act, off_zero, zero_bytes, total;
};

// gu_width: 2F, or 0 for an MLP without a gate (its up-projection goes straight to act: no gate buffer)
inline VarlenWs varlen_plan(int n_rows, size_t H, size_t qkv_width, size_t vt_width, size_t ctx_width, size_t gu_width, size_t F,
                            size_t zero_floats) {
    VarlenWs e{};
    const size_t T = ((size_t)n_rows + 255) / 256 * 256;
    WsPlanner ws;
    e.off_ha = ws.take(T * H * 2);
    e.off_hb = ws.take(T * H * 2);
    e.off_x = ws.take(T * H * 2);
    e.off_qkv = ws.take(T * qkv_width * 2);
    e.off_vt = ws.take(T * vt_width * 2);
    e.off_ctx = ws.take(T * ctx_width * 2);
    e.off_gu = ws.take(T * gu_width * 2);
    e.off_act = ws.take(T * F * 2);
    e.zero_bytes = zero_floats * 4;
    e.off_zero = ws.take(e.zero_bytes);
    e.total = ws.off;
    return e;
}

// the packed batch of one forward
struct PackedSeqs {
    const int32_t *seq_start, *seq_len;
    int n_seq, n_rows, max_len;
};

// how a layer's QKV projection is stored: q | k rows [T][2H] plus V in the V8 layout [T/8][H][8], written by the GEMM's epilogue
// (TT_EPI_QKV), or one packed row [T][qkv width] of which the family's next launch copies V out (TT_EPI_BIAS)
enum class QkvForm { SplitV8, Packed };

// ---- shape checks, each called with the family's prefix ("decoder", "t5", ...) -----------------------------------------------------
// the row ops hold a row of up to 1024 values, and the scan takes vectors up to that width (`name`: what the family calls it)
inline int check_hidden(const char* family, int hidden, const char* name = "hidden") {
    if (hidden <= 0 || hidden % 128 || hidden > 1024) {
        tt_set_error("%s: %s=%d must be a multiple of 128 and <= 1024 (the scan's limit)", family, name, hidden);
        return TT_E_UNSUPPORTED;
    }
    return TT_OK;
}

// grouped-query heads of width d0 (or d1, where the family's attention has two instantiations)
inline int check_gqa_heads(const char* family, int heads, int kv_heads, int head_dim, int d0, int d1 = 0) {
    if (head_dim != d0 && (d1 == 0 || head_dim != d1)) {
        if (d1)
            tt_set_error("%s: head_dim=%d not in {%d, %d}", family, head_dim, d0, d1);
        else
            tt_set_error("%s: head_dim=%d (supported: %d)", family, head_dim, d0);
        return TT_E_UNSUPPORTED;
    }
    TT_CHECK_ARG(heads > 0 && kv_heads > 0 && heads % kv_heads == 0, "%s: heads=%d is not a multiple of kv_heads=%d", family, heads,
                 kv_heads);
    return TT_OK;
}

// the GEMM tiles: the fused q | k | v projection is 128 columns wide, the output projection's K and the gated MLP's F 64
inline int check_qkv_width(const char* family, int heads, int kv_heads, int head_dim, int ffn) {
    if (((heads + 2 * kv_heads) * head_dim) % 128 || (heads * head_dim) % 64 || ffn <= 0 || ffn % 64) {
        tt_set_error("%s: (heads + 2 kv_heads) * head_dim = %d must be a multiple of 128, heads * head_dim and ffn=%d of 64", family,
                     (heads + 2 * kv_heads) * head_dim, ffn);
        return TT_E_UNSUPPORTED;
    }
    return TT_OK;
}

// the batch arguments every packed forward takes (`family`: "a decoder", "ModernBERT"; `need`: the plan's total -- the caller
// computes it before n_rows is checked here: unsigned arithmetic, and not looked at unless n_rows passes)
inline int check_packed_forward_args(const char* what, const char* family, const int32_t* ids, const int32_t* pos, const int32_t* type_ids,
                                     const int32_t* seq_start, const int32_t* seq_len, int n_seq, int n_rows, int max_len,
                                     const void* hidden_out, const void* workspace, size_t workspace_bytes, size_t need) {
    TT_CHECK_ARG(type_ids == nullptr, "%s has no token types: type_ids must be NULL", family);
    TT_CHECK_ARG(n_rows > 0 && (n_rows % 128 == 0 || (n_rows < 256 && n_rows % 64 == 0)),
                 "n_rows=%d must be a positive multiple of 128 (or 64 / 192)", n_rows);
    TT_CHECK_ARG(n_seq > 0 && max_len > 0 && max_len <= n_rows, "n_seq=%d max_len=%d", n_seq, max_len);
    TT_CHECK_ARG(ids && pos && seq_start && seq_len && hidden_out, "null pointer");
    return tt_check_workspace(what, workspace, workspace_bytes, need);
}

// the operands of the attention building blocks on the one-wave tile with as many KV heads as query heads (`what`: "windowed
// attention", "ALiBi attention"; `operands`: the entry point's own pointers are present): heads of 64, 16-byte Q / K / V reads,
// 8-byte output stores, every head's columns inside a row
inline int check_attention_layout(const char* what, bool operands, const void* qkv, int ld, int q_col0, int k_col0, const void* vt,
                                  int ldvt, const void* out, int ld_out, const int32_t* seq_start, const int32_t* seq_len, int n_seq,
                                  int n_rows, int heads, int head_dim, int max_len) {
    if (head_dim != 64) {
        tt_set_error("%s: head_dim=%d (supported: 64)", what, head_dim);
        return TT_E_UNSUPPORTED;
    }
    TT_CHECK_ARG(qkv && vt && out && seq_start && seq_len && operands, "null pointer");
    TT_CHECK_ARG(heads > 0 && n_seq > 0 && max_len > 0 && n_rows > 0 && n_rows % 8 == 0 && max_len <= n_rows,
                 "heads=%d n_seq=%d n_rows=%d max_len=%d", heads, n_seq, n_rows, max_len);
    TT_CHECK_ARG(ld % 8 == 0 && q_col0 % 8 == 0 && k_col0 % 8 == 0 && q_col0 >= 0 && k_col0 >= 0 && ld_out % 4 == 0 &&
                     ld >= std::max(q_col0, k_col0) + heads * 64 && ld_out >= heads * 64 && ldvt >= 8 * heads * 64 && ldvt % 8 == 0,
                 "ld=%d q_col0=%d k_col0=%d ld_out=%d ldvt=%d", ld, q_col0, k_col0, ld_out, ldvt);
    return TT_OK;
}

}  // namespace
