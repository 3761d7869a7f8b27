// Maximal marginal relevance over the scan's hits (include/tt_hip.h, "MMR: diversified top-k").
//   tt_mmr_select   per query: G = pairwise dot products of the candidates' corpus rows (mmr_gram_kernel), then the greedy
//                   selection v = lambda rel - (1 - lambda) pen over them (mmr_greedy_kernel), stream-ordered, no host step between
// The candidates are whatever tt_scan_topk wrote: corpus rows in the scan's order with their scores, padding < 0.
//
// The Gram tiles are one-wave MFMA tiles without LDS staging, as colbert.hip's MaxSim: a lane's operand fragment of
// mfma_f32_16x16x32_bf16 is 16 contiguous bytes of one gathered row (row on lane & 15, K offset 8 (lane >> 4)); the accumulator of
// lane l holds rows 4 (l >> 4) + i, i = 0..3, of column l & 15.  bf16 only: the scan's corpus has no fp16 twin.
#include "common.h"

#include <limits.h>
#include <math.h>

#include <algorithm>

namespace {

constexpr int kMaxCand = 1024;
constexpr int kGramWaves = 4;        // independent 16x16 tiles a workgroup works on (one per wave, one per SIMD)
constexpr int kGramStep = 4;         // 32-wide K steps loaded ahead as one group (dim is a multiple of 128)
constexpr int kGreedyThreads = 256;  // at most kMaxCand / kGreedyThreads = 4 candidates per thread
constexpr int kPerThread = kMaxCand / kGreedyThreads;

// the corpus row of a list entry, or -1: padding (entry < 0), or a row outside the matrix -- never read
__device__ __forceinline__ int64_t mmr_row(int32_t entry, int32_t idx_base, int64_t n_rows) {
    if (entry < 0) return -1;
    const int64_t r = (int64_t)entry - idx_base;
    return r >= 0 && r < n_rows ? r : -1;
}

// ---- pairwise similarity ------------------------------------------------------------------------------------------------------
// Query q's candidates in blocks of 16 list positions; wave (workgroup, w) takes the block pair t = 4 workgroup + w of the pairs
// (bi <= bj) in row-major order of the upper triangle.  A rows = the 16 candidates of block bi, B columns = those of block bj; the
// chain over kk = 0 .. dim/32 - 1 runs from a zero accumulator, one MFMA per kk, so an entry is a function of its two corpus rows
// alone: not of the list position, of n_cand, of the query, or of the wave.  A padding lane loads row 0 (the host launches nothing
// for an empty matrix) and feeds zeros instead: its entries come out +0, and the loads stay unconditional, so they can be counted.
// A pair above the diagonal is written to both places from the one value; a diagonal block writes its r <= c half to both places.
// The next group of kGramStep K steps is loaded before the current group's MFMAs are issued.  No LDS, no barrier.
__global__ __launch_bounds__(64 * kGramWaves) void mmr_gram_kernel(const uint16_t* __restrict__ corpus, int64_t n_rows, int dim,
                                                                   const int32_t* __restrict__ cand, int n_cand, int ppad,
                                                                   int32_t idx_base, int n_pairs, int wg_per_query,
                                                                   float* __restrict__ ws) {
    const int q = blockIdx.x / wg_per_query;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int t = (blockIdx.x % wg_per_query) * kGramWaves + wave;
    if (t >= n_pairs) return;   // (wave-uniform)
    const int nb = ppad >> 4;
    int bi = 0, rem = t;
    while (rem >= nb - bi) {
        rem -= nb - bi;
        ++bi;
    }
    const int bj = bi + rem;
    const int lane = threadIdx.x & 63, c = lane & 15, g = lane >> 4;
    const int32_t* cq = cand + (size_t)q * n_cand;
    const int pa = 16 * bi + c, pb = 16 * bj + c;
    const int64_t ra = pa < n_cand ? mmr_row(cq[pa], idx_base, n_rows) : -1;
    const int64_t rb = pb < n_cand ? mmr_row(cq[pb], idx_base, n_rows) : -1;
    const uint16_t* abase = corpus + (size_t)(ra < 0 ? 0 : ra) * dim + 8 * g;
    const uint16_t* bbase = corpus + (size_t)(rb < 0 ? 0 : rb) * dim + 8 * g;
    const uint4 zero4 = uint4{0u, 0u, 0u, 0u};
    auto load = [&](uint4(&a)[kGramStep], uint4(&b)[kGramStep], int k0) {
#pragma unroll
        for (int i = 0; i < kGramStep; ++i) {
            a[i] = *reinterpret_cast<const uint4*>(abase + (size_t)(k0 + i) * 32);
            b[i] = *reinterpret_cast<const uint4*>(bbase + (size_t)(k0 + i) * 32);
        }
    };
    const int nk = dim >> 5;
    uint4 a0[kGramStep], b0[kGramStep], a1[kGramStep], b1[kGramStep];
    f32x4 s = f32x4{0.f, 0.f, 0.f, 0.f};
    load(a0, b0, 0);
    for (int k0 = 0; k0 < nk; k0 += kGramStep) {   // (wave-uniform)
        // (the last turn loads its own group again rather than branch: with a branch here the compiler waits for every load in flight)
        load(a1, b1, min(k0 + kGramStep, nk - kGramStep));
#pragma unroll
        for (int i = 0; i < kGramStep; ++i)
            s = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, ra >= 0 ? a0[i] : zero4),
                                                        __builtin_bit_cast(bf16x8, rb >= 0 ? b0[i] : zero4), s, 0, 0, 0);
#pragma unroll
        for (int i = 0; i < kGramStep; ++i) {
            a0[i] = a1[i];
            b0[i] = b1[i];
        }
    }
    float* G = ws + (size_t)q * ppad * ppad;
    if (bi != bj) {
#pragma unroll
        for (int i = 0; i < 4; ++i) G[(size_t)(16 * bi + 4 * g + i) * ppad + 16 * bj + c] = s[i];
        *reinterpret_cast<float4*>(G + (size_t)(16 * bj + c) * ppad + 16 * bi + 4 * g) = float4{s[0], s[1], s[2], s[3]};
    } else {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int r = 4 * g + i;
            if (r <= c) {
                G[(size_t)(16 * bi + r) * ppad + 16 * bi + c] = s[i];
                G[(size_t)(16 * bi + c) * ppad + 16 * bi + r] = s[i];
            }
        }
    }
}

// ---- greedy selection ---------------------------------------------------------------------------------------------------------
// a beats b: b is "nothing", or a's value is larger, or equal (-0 == +0) at a lower list position.  NaN values never get here.
__device__ __forceinline__ bool mmr_beats(float va, int pa, float vb, int pb) {
    return pa != INT_MAX && (pb == INT_MAX || va > vb || (va == vb && pa < pb));
}

// lr - oml * pen in two roundings.  The library is built with -ffp-contract=fast and __fmul_rn / __fsub_rn are a plain * and - to the
// compiler: the empty asm keeps the product out of a v_fma_f32 (rowops.hip's mul_then_add does the same).
__device__ __forceinline__ float mmr_value(float lr, float oml, float pen) {
    float p = __fmul_rn(oml, pen);
    asm("" : "+v"(p));
    return __fsub_rn(lr, p);
}

// One workgroup per query; thread t owns list positions t + 256 j.  lambda rel, pen and the open flags (valid and not yet taken) of
// its candidates live in registers.  Per step: every thread finds the best of its own (positions upward, strict >), a butterfly over
// the wave reduces the pair (value, position), lane 0 of each wave posts it to LDS (two slots, alternating: one barrier per step)
// and every thread folds the waves' pairs in wave order, so all agree on the pick.  Its owner writes the four outputs; then every
// thread reads its entries of row `pick` of G.  
__global__ __launch_bounds__(kGreedyThreads) void mmr_greedy_kernel(const int32_t* __restrict__ cand, const float* __restrict__ rel,
                                                                    int n_cand, int ppad, int k, float lambda, int penalty,
                                                                    int32_t idx_base, int64_t n_rows, const float* __restrict__ ws,
                                                                    float* __restrict__ out_mmr, float* __restrict__ out_rel,
                                                                    int32_t* __restrict__ out_idx, int32_t* __restrict__ out_pos) {
    __shared__ float post_v[2][kGreedyThreads / 64];
    __shared__ int post_p[2][kGreedyThreads / 64];
    const int q = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, n_waves = blockDim.x >> 6;
    const int32_t* cq = cand + (size_t)q * n_cand;
    const float* rq = rel + (size_t)q * n_cand;
    const float* G = ws + (size_t)q * ppad * ppad;
    const size_t out0 = (size_t)q * k;
    const float oml = __fsub_rn(1.0f, lambda);
    float lr[kPerThread], rl[kPerThread], pen[kPerThread];
    int32_t ent[kPerThread];
    bool open[kPerThread];
#pragma unroll
    for (int j = 0; j < kPerThread; ++j) {
        const int d = tid + kGreedyThreads * j;
        ent[j] = d < n_cand ? cq[d] : -1;
        open[j] = d < n_cand && mmr_row(ent[j], idx_base, n_rows) >= 0;
        rl[j] = open[j] ? rq[d] : 0.f;
        lr[j] = __fmul_rn(lambda, rl[j]);
        pen[j] = 0.f;
    }
    for (int s = 0; s < k; ++s) {   // (workgroup-uniform)
        float bv = 0.f;
        int bp = INT_MAX;
#pragma unroll
        for (int j = 0; j < kPerThread; ++j) {
            const float v = s == 0 ? lr[j] : mmr_value(lr[j], oml, pen[j]);
            if (open[j] && v == v && (bp == INT_MAX || v > bv)) {
                bv = v;
                bp = tid + kGreedyThreads * j;
            }
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const float ov = __shfl_xor(bv, o, 64);
            const int op = __shfl_xor(bp, o, 64);
            if (mmr_beats(ov, op, bv, bp)) {
                bv = ov;
                bp = op;
            }
        }
        if (n_waves > 1) {
            if (lane == 0) {
                post_v[s & 1][wave] = bv;
                post_p[s & 1][wave] = bp;
            }
            __syncthreads();
            bv = post_v[s & 1][0];
            bp = post_p[s & 1][0];
            for (int w = 1; w < n_waves; ++w) {
                const float ov = post_v[s & 1][w];
                const int op = post_p[s & 1][w];
                if (mmr_beats(ov, op, bv, bp)) {
                    bv = ov;
                    bp = op;
                }
            }
        }
        if (bp == INT_MAX) {   // nothing left to pick: the rest is padding
            for (int o = s + tid; o < k; o += blockDim.x) {
                out_mmr[out0 + o] = -INFINITY;
                out_rel[out0 + o] = -INFINITY;
                out_idx[out0 + o] = -1;
                out_pos[out0 + o] = -1;
            }
            return;
        }
#pragma unroll
        for (int j = 0; j < kPerThread; ++j) {
            if (bp == tid + kGreedyThreads * j) {
                out_mmr[out0 + s] = bv;
                out_rel[out0 + s] = rl[j];
                out_idx[out0 + s] = ent[j];
                out_pos[out0 + s] = bp;
                open[j] = false;
            }
        }
        if (s + 1 < k) {
            const float* grow = G + (size_t)bp * ppad;
#pragma unroll
            for (int j = 0; j < kPerThread; ++j) {
                const int d = tid + kGreedyThreads * j;
                if (d < n_cand) {
                    const float gv = grow[d];
                    pen[j] = (penalty == 1 || s == 0) ? gv : fmaxf(pen[j], gv);
                }
            }
        }
    }
}

inline int mmr_ppad(int n_cand) { return (n_cand + 15) / 16 * 16; }

}  // namespace

extern "C" {

size_t tt_mmr_workspace_bytes(int n_queries, int n_cand) {
    if (n_queries < 0 || n_cand < 1 || n_cand > kMaxCand) return 0;
    const size_t pp = (size_t)mmr_ppad(n_cand);
    return (size_t)n_queries * pp * pp * sizeof(float);
}

int tt_mmr_select(const void* corpus_bf16, int64_t n_rows, int dim, const int32_t* cand, const float* rel, int n_queries, int n_cand,
                  int k, float lambda, int penalty, int32_t idx_base, float* out_mmr, float* out_rel, int32_t* out_idx,
                  int32_t* out_pos, void* workspace, size_t workspace_bytes, void* stream) {
    if (dim <= 0 || dim % 128 || dim > 1024) {
        tt_set_error("tt_mmr_select: dim=%d must be a multiple of 128 and <= 1024", dim);
        return TT_E_UNSUPPORTED;
    }
    if (n_cand < 1 || n_cand > kMaxCand || k < 1 || k > n_cand || (penalty != 0 && penalty != 1)) {
        tt_set_error("tt_mmr_select: n_cand=%d (1 .. %d), k=%d (1 .. n_cand), penalty=%d (0: maximum, 1: last pick)", n_cand, kMaxCand,
                     k, penalty);
        return TT_E_UNSUPPORTED;
    }
    TT_CHECK_ARG(lambda >= 0.f && lambda <= 1.f, "tt_mmr_select: lambda=%g outside [0, 1]", (double)lambda);   // (a NaN fails both)
    TT_CHECK_ARG(n_queries >= 0 && n_rows >= 0, "tt_mmr_select: n_queries=%d n_rows=%lld", n_queries, (long long)n_rows);
    if (n_queries == 0) return TT_OK;
    TT_CHECK_ARG(corpus_bf16 && cand && rel && out_mmr && out_rel && out_idx && out_pos, "tt_mmr_select: null pointer");
    const size_t need = tt_mmr_workspace_bytes(n_queries, n_cand);
    if (!workspace || workspace_bytes < need) {
        tt_set_error("tt_mmr_select: workspace %zu < required %zu bytes", workspace_bytes, need);
        return TT_E_WORKSPACE;
    }
    TT_CHECK_ARG((uintptr_t)workspace % 16 == 0, "tt_mmr_select: workspace must be 16-byte aligned");
    const int ppad = mmr_ppad(n_cand), nb = ppad / 16;
    const int n_pairs = nb * (nb + 1) / 2;
    const int wg_per_query = (n_pairs + kGramWaves - 1) / kGramWaves;
    const int64_t grid = (int64_t)n_queries * wg_per_query;
    TT_CHECK_ARG(grid <= INT_MAX, "tt_mmr_select: n_queries=%d x n_cand=%d is more than one launch holds", n_queries, n_cand);
    hipStream_t st = (hipStream_t)stream;
    TtProfScope prof(TT_K_ROWOPS, st);
    if (n_rows > 0) {   // (an empty matrix: every entry is padding, nothing is picked and no entry of G is read)
        hipLaunchKernelGGL(mmr_gram_kernel, dim3((unsigned)grid), dim3(64 * kGramWaves), 0, st, (const uint16_t*)corpus_bf16, n_rows,
                           dim, cand, n_cand, ppad, idx_base, n_pairs, wg_per_query, (float*)workspace);
        TT_CHECK_LAUNCH();
    }
    const int threads = std::min(kGreedyThreads, (n_cand + 63) / 64 * 64);
    hipLaunchKernelGGL(mmr_greedy_kernel, dim3((unsigned)n_queries), dim3(threads), 0, st, cand, rel, n_cand, ppad, k, lambda, penalty,
                       idx_base, n_rows, (const float*)workspace, out_mmr, out_rel, out_idx, out_pos);
    TT_CHECK_LAUNCH();
    return TT_OK;
}

}  // extern "C"
