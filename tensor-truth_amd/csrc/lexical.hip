// Lexical (sparse) retrieval with BGE-M3's second head (include/tt_hip.h, "Lexical weights and hybrid scoring").
//   tt_lexical_weights[_f16|_f32]  per-token weights relu(<w, h_i> + b) of a packed hidden state -> per sequence, its distinct kept
//                                  token ids in ascending order, each with the maximum weight over its occurrences
//   tt_lexical_score               lex[q][c] = sum over shared ids of q_w * d_w, the dense dot product and their weighted mean, over
//                                  entries that already sit in device memory
//   tt_lexical_scan_topk           that lexical score for every stored document, then the library's exact selection (select.hip)
//   tt_hybrid_scan_topk            the hybrid score of tt_lexical_score for every stored document in one read of the store per pass
//                                  of queries, then the same selection
//   tt_lexical_score_lists         (internal, scan.h) the scan's lexical scores over per-query candidate lists, for postings.hip
//
// Compiled twice like the encoder path (common.h TT_F16): the bf16 object holds everything; the fp16 object only
// tt_lexical_weights (as tt_lexical_weights_f16, f16_names.h), the one entry point whose operands are 16-bit hidden states.
#include "common.h"
#include "scan.h"

#include <limits.h>

#include <algorithm>

namespace {

typedef unsigned long long u64;

constexpr int kMaxH = 1024;          // hidden sizes: multiples of 128 up to here (the dense vectors of tt_lexical_score as well)
constexpr int kMaxSeqLen = 8192;     // BGE_M3.max_seq_len: 8192 (id, weight) pairs are 64 KiB of LDS
constexpr int kDotWaves = 4;         // waves of a token-weight workgroup
constexpr int kDotRows = 16;         // rows of one sequence a token-weight workgroup takes
constexpr u64 kNoKey = ~0ull;        // sorts behind every kept (id, weight)

struct Skip4 { int32_t a, b, c, d; };

// ---- token weights ------------------------------------------------------------------------------------------------------------
// One wave per token row.  Lane l holds elements 128 c + 2 l, + 1 of the row for c = 0 .. H / 128 - 1 and adds their products
// with w in that order in fp32 (fmaf); the 64 partial sums meet in wave_sum's butterfly.  The order is a function of H alone, so a
// row's pre-activation is the same bits wherever the row sits.  raw[row] = sum + bias for the rows of sequences only.
template <bool F32>
__device__ __forceinline__ f32x2 load_pair(const void* base, size_t elem) {
    if constexpr (F32) {
        const float2 v = *reinterpret_cast<const float2*>(static_cast<const float*>(base) + elem);
        return f32x2{v.x, v.y};
    } else {
        const uint32_t u = *reinterpret_cast<const uint32_t*>(static_cast<const uint16_t*>(base) + elem);
        return f32x2{elo(u), ehi(u)};
    }
}

template <bool F32>
__global__ __launch_bounds__(64 * kDotWaves) void lexical_dot_kernel(const void* __restrict__ hidden, int ld, int H,
                                                                     const void* __restrict__ w, float bias,
                                                                     const int32_t* __restrict__ seq_start,
                                                                     const int32_t* __restrict__ seq_len, int len_cap,
                                                                     int n_rows, float* __restrict__ raw) {
    const int b = blockIdx.y;
    const int s0 = seq_start[b], L = min(min(max(seq_len[b], 0), len_cap), n_rows - s0);   // (no row at or behind n_rows is touched)
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int r0 = blockIdx.x * kDotRows;
    if (s0 < 0 || r0 >= L) return;   // (workgroup-uniform)
    const int chunks = H >> 7;
    f32x2 wf[kMaxH / 128];
#pragma unroll
    for (int c = 0; c < kMaxH / 128; ++c) wf[c] = c < chunks ? load_pair<F32>(w, (size_t)128 * c + 2 * lane) : f32x2{0.f, 0.f};
    for (int r = r0 + wave; r < min(r0 + kDotRows, L); r += kDotWaves) {   // (wave-uniform)
        const size_t row = (size_t)(s0 + r) * ld;
        float acc = 0.f;
#pragma unroll
        for (int c = 0; c < kMaxH / 128; ++c) {
            if (c < chunks) {
                const f32x2 h = load_pair<F32>(hidden, row + 128 * c + 2 * lane);
                acc = fmaf(h.x, wf[c].x, acc);
                acc = fmaf(h.y, wf[c].y, acc);
            }
        }
        acc = wave_sum(acc) + bias;
        if (lane == 0) raw[s0 + r] = acc;
    }
}

// ---- per-sequence sort and dedup in LDS ------------------------------------------------------------------------------------------
// One workgroup per sequence.  Token i becomes the 64-bit key (id << 32 | bits of its weight) -- a positive float's bits order as
// the float does -- or kNoKey when it is not kept (one of the four ids left out, a negative id, a weight <= 0 or NaN).  A bitonic
// sort over the next power of two >= the sequence's length puts equal ids side by side with the largest weight last; an element is
// written when its successor carries another id: the maximum over occurrences, exactly.  The write position is an exclusive prefix
// count over the sorted order, so ids come out ascending.  NCAP keys of 8 bytes: 0.5 / 4 / 16 / 64 KiB of LDS per workgroup.
template <int NCAP>
struct DedupShape {
    static constexpr int threads = NCAP / 2 < 1024 ? (NCAP / 2 < 64 ? 64 : NCAP / 2) : 1024;
};

template <int NCAP>
__global__ __launch_bounds__(DedupShape<NCAP>::threads) void lexical_dedup_kernel(const int32_t* __restrict__ ids,
                                                                                  const int32_t* __restrict__ seq_start,
                                                                                  const int32_t* __restrict__ seq_len, int n_rows,
                                                                                  Skip4 skip,
                                                                                  int32_t* __restrict__ out_terms,
                                                                                  float* __restrict__ out_weights,
                                                                                  int32_t* __restrict__ out_nnz) {
    constexpr int T = DedupShape<NCAP>::threads;
    __shared__ u64 key[NCAP];
    __shared__ int cnt[2][T];
    const int b = blockIdx.x, tid = threadIdx.x;
    const int s0 = seq_start[b], L = min(min(max(seq_len[b], 0), NCAP), n_rows - s0);
    if (s0 < 0 || L <= 0) {   // (workgroup-uniform)
        if (tid == 0) out_nnz[b] = 0;
        return;
    }
    int n = 2;
    while (n < L) n <<= 1;
    // out_weights holds the pre-activations of lexical_dot_kernel: every one is read here, before the barrier of the first stage
    for (int i = tid; i < n; i += T) {
        u64 k = kNoKey;
        if (i < L) {
            const int32_t id = ids[s0 + i];
            const float t = out_weights[s0 + i];
            if (id >= 0 && id != skip.a && id != skip.b && id != skip.c && id != skip.d && t > 0.f)
                k = ((u64)(uint32_t)id << 32) | (u64)__float_as_uint(t);
        }
        key[i] = k;
    }
    __syncthreads();
    for (int size = 2; size <= n; size <<= 1) {
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            for (int p = tid; p < (n >> 1); p += T) {
                const int lo = 2 * p - (p & (stride - 1)), hi = lo + stride;
                const bool up = (lo & size) == 0;
                const u64 a = key[lo], c = key[hi];
                if ((a > c) == up) {
                    key[lo] = c;
                    key[hi] = a;
                }
            }
            __syncthreads();
        }
    }
    // thread t owns the sorted positions [t * per, (t + 1) * per)
    const int per = (n + T - 1) / T;
    const int i0 = min(tid * per, n), i1 = min(i0 + per, n);
    int mine = 0;
    for (int i = i0; i < i1; ++i) {
        const u64 k = key[i];
        mine += (k != kNoKey && (i + 1 == n || (uint32_t)(key[i + 1] >> 32) != (uint32_t)(k >> 32))) ? 1 : 0;
    }
    cnt[0][tid] = mine;
    __syncthreads();
    int cur = 0;
    for (int off = 1; off < T; off <<= 1) {   // inclusive prefix sums
        const int v = cnt[cur][tid] + (tid >= off ? cnt[cur][tid - off] : 0);
        cnt[cur ^ 1][tid] = v;
        cur ^= 1;
        __syncthreads();
    }
    const int nnz = cnt[cur][T - 1];
    int pos = cnt[cur][tid] - mine;
    for (int i = i0; i < i1; ++i) {
        const u64 k = key[i];
        if (k != kNoKey && (i + 1 == n || (uint32_t)(key[i + 1] >> 32) != (uint32_t)(k >> 32))) {
            out_terms[s0 + pos] = (int32_t)(uint32_t)(k >> 32);
            out_weights[s0 + pos] = __uint_as_float((uint32_t)k);
            ++pos;
        }
    }
    for (int i = nnz + tid; i < L; i += T) {
        out_terms[s0 + i] = -1;
        out_weights[s0 + i] = 0.f;
    }
    if (tid == 0) out_nnz[b] = nnz;
}

#if !TT_F16
// ---- lexical, dense and hybrid scores ------------------------------------------------------------------------------------------
// A workgroup stages one query's entry (<= 512 ids and weights, 4 KiB) in LDS; each of its waves then takes candidates of that
// query, kScoreWaves apart.  A document's entry streams from memory once: lane l takes its ids l, l + 64, ..., finds each among the
// query's by bisection and adds q_w * d_w to its own fp32 sum in that order; wave_sum's butterfly adds the 64 sums.  The dense part
// does the same over dim (lane l: elements 128 c + 2 l, + 1; bf16 operands, fp32 fmaf).  Nothing depends on which other pairs the
// launch holds.  `dead`: what a negative candidate or a tombstone (d_nnz < 0) writes -- -inf for tt_lexical_score, NaN in the
// scan's workspace, where the selection must never return it.
constexpr int kScoreWaves = 4;
constexpr int kMaxQueryNnz = 512, kMaxDocNnz = 8192;

// the hybrid score of one pair, (w_dense * dense + w_lex * lex) / (w_dense + w_lex): ONE expression, shared by lexical_score_kernel
// and hybrid_scan_kernel.  The fusion is spelled out -- the dense product rounded, the lexical one fused into the addition, which is
// what the compiler made of the plain expression in lexical_score_kernel -- because left to -ffp-contract=fast the choice of the
// fused product depends on the code around the expression: inlined into hybrid_scan_kernel the same line fused the OTHER product,
// one ulp apart wherever lex != 0 (measured, tests/test_hybrid_scan_gpu.py).
__device__ __forceinline__ float hybrid_mix(float w_dense, float dense, float w_lex, float lex) {
    return fmaf(w_lex, lex, w_dense * dense) / (w_dense + w_lex);
}

__global__ __launch_bounds__(64 * kScoreWaves) void lexical_score_kernel(
    const int32_t* __restrict__ q_terms, const float* __restrict__ q_weights, const int32_t* __restrict__ q_start,
    const int32_t* __restrict__ q_nnz, const int32_t* __restrict__ d_terms, const float* __restrict__ d_weights,
    const int64_t* __restrict__ d_start, const int32_t* __restrict__ d_nnz, const int32_t* __restrict__ cand,
    const int32_t* __restrict__ cand_cnt, int64_t cand_stride, int n_cand, int64_t out_stride, const uint16_t* __restrict__ q_dense,
    const uint16_t* __restrict__ d_dense, int dim, float w_dense, float w_lex, float dead, float* __restrict__ out_lex,
    float* __restrict__ out_dense, float* __restrict__ out_hybrid) {
    __shared__ int32_t qt[kMaxQueryNnz];
    __shared__ float qw[kMaxQueryNnz];
    const int q = blockIdx.y;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int nq = min(max(q_nnz[q], 0), kMaxQueryNnz);
    const int qs = q_start[q];
    for (int i = threadIdx.x; i < nq; i += 64 * kScoreWaves) {
        qt[i] = q_terms[qs + i];
        qw[i] = q_weights[qs + i];
    }
    __syncthreads();
    const int chunks = dim >> 7;
    f32x2 qd[kMaxH / 128];
#pragma unroll
    for (int c = 0; c < kMaxH / 128; ++c)
        qd[c] = (q_dense && c < chunks) ? load_pair<false>(q_dense, (size_t)q * dim + 128 * c + 2 * lane) : f32x2{0.f, 0.f};
    // cand_cnt (postings.hip: a query's own list length, known on the device only) cuts the walk short; it changes which pairs are
    // scored, never a pair's bits
    const int n_mine = cand_cnt ? min(max(cand_cnt[q], 0), n_cand) : n_cand;
    for (int ci = blockIdx.x * kScoreWaves + wave; ci < n_mine; ci += gridDim.x * kScoreWaves) {   // (wave-uniform)
        const int doc = cand ? cand[(size_t)q * cand_stride + ci] : ci;
        const size_t o = (size_t)q * out_stride + ci;
        const int dn_raw = doc >= 0 ? d_nnz[doc] : -1;
        if (dn_raw < 0) {
            if (lane == 0) {
                out_lex[o] = dead;
                if (q_dense) {
                    out_dense[o] = dead;
                    out_hybrid[o] = dead;
                }
            }
            continue;
        }
        const int dn = min(dn_raw, kMaxDocNnz);
        const int64_t ds = d_start[doc];
        float acc = 0.f;
        for (int j = lane; j < dn; j += 64) {
            const int32_t t = d_terms[ds + j];
            int lo = 0, hi = nq;   // first query position whose id is >= t
            while (lo < hi) {
                const int mid = (lo + hi) >> 1;
                if (qt[mid] < t) lo = mid + 1; else hi = mid;
            }
            if (lo < nq && qt[lo] == t) acc = fmaf(qw[lo], d_weights[ds + j], acc);
        }
        const float lex = wave_sum(acc);
        if (!q_dense) {
            if (lane == 0) out_lex[o] = lex;
            continue;
        }
        float dacc = 0.f;
#pragma unroll
        for (int c = 0; c < kMaxH / 128; ++c) {
            if (c < chunks) {
                const f32x2 d = load_pair<false>(d_dense, (size_t)doc * dim + 128 * c + 2 * lane);
                dacc = fmaf(qd[c].x, d.x, dacc);
                dacc = fmaf(qd[c].y, d.y, dacc);
            }
        }
        const float dense = wave_sum(dacc);
        if (lane == 0) {
            out_lex[o] = lex;
            out_dense[o] = dense;
            out_hybrid[o] = hybrid_mix(w_dense, dense, w_lex, lex);
        }
    }
}

// ---- the hybrid score over the whole store ------------------------------------------------------------------------------------
// tt_hybrid_scan_topk's scoring pass: every document is read ONCE and scored against every query of the pass.  A persistent grid
// (kHybWgPerCu workgroups per compute unit) of four-wave workgroups; a wave owns whole documents, taken in a static grid-stride
// walk over runs of kHybRun consecutive document numbers -- no atomics, nothing crosses a wave, so which wave scores a document
// cannot matter.
//   Queries: the pass's entries (ids and weights as lexical_score_kernel stores them, QCAP slots per query: 64 or 512) and dense
//     rows are staged once per workgroup in LDS.  A dense row stays bf16, as it lies in memory: word 64 c + l of a row is the pair
//     (128 c + 2 l, + 1) that lane l owns in chunk c, so a wave's read of one query's chunk covers 256 consecutive bytes
//     (conflict-free); the pair is converted to fp32 where it is used.
//   Documents: a run's live documents are loaded once -- the dense row as <= 8 converted register pairs per lane, entries lane,
//     lane + 64, .. lane + 192 of the CSR entry (its first 256 ids and weights) as kHybRegs more pairs -- before the first of them is
//     scored, and reused against every query of the pass.  Entries 256 and up stream from memory per query (the caches hold
//     them), in lexical_score_kernel's order.  The run's d_nnz and d_start were fetched one step of the walk earlier.
//   Per pair the two sums are lexical_score_kernel's: lane l adds the matches of entries l, l + 64, ... by fmaf(q_w, d_w, acc), the
//     products of elements 128 c + 2 l, + 1 for ascending c by fmaf, x then y; wave_sum joins the lanes.  The bisections of a
//     lane's register entries run side by side (the same comparisons as one after the other; their LDS reads overlap); the
//     matches are added in entry order.  Every lane then holds the
//     pair's sums; lane kHybRun * q + r keeps those of (query q of the pass, document r of the run), mixes them once (hybrid_mix)
//     and stores: a query's run is 16 consecutive bytes of its workspace row.  A tombstone (d_nnz < 0) is not read and writes NaN.
constexpr int kHybWaves = 4;        // waves per workgroup
constexpr int kHybRun = 4;          // consecutive documents a wave takes per step of its walk
constexpr int kHybRegs = 4;         // entries of a document a lane holds in registers: its first 256 ids and weights in all
constexpr int kHybWgPerCu = 3;      // workgroups the grid holds per compute unit (3 x <= 49 KB of its 160 KB of LDS)
constexpr int kHybShort = 64;       // the short class of max_q_nnz_host: a query's LDS slot holds 64 ids; the long one kMaxQueryNnz
// queries per pass: kHybRun x this many (query, document) slots are the wave's 64 lanes, or half of them
template <int QCAP>
struct HybPass {
    static constexpr int queries = QCAP <= kHybShort ? 16 : 8;
};

// acc + q_w * d_w if the query holds id t (lexical_score_kernel's bisection and fmaf)
__device__ __forceinline__ float hybrid_match(const int32_t* qt, const float* qw, int nq, int32_t t, const float* dw, float acc) {
    int lo = 0, hi = nq;   // first query position whose id is >= t
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (qt[mid] < t) lo = mid + 1; else hi = mid;
    }
    if (lo < nq && qt[lo] == t) acc = fmaf(qw[lo], *dw, acc);
    return acc;
}

// DC: the dense row's chunks of 128 elements the registers hold (2, 4 or 8: dim <= 256, 512, 1024); QCAP: ids per query slot
template <int DC, int QCAP>
__global__ __launch_bounds__(64 * kHybWaves) void hybrid_scan_kernel(
    const int32_t* __restrict__ q_terms, const float* __restrict__ q_weights, const int32_t* __restrict__ q_start,
    const int32_t* __restrict__ q_nnz, int n_q, const int32_t* __restrict__ d_terms, const float* __restrict__ d_weights,
    const int64_t* __restrict__ d_start, const int32_t* __restrict__ d_nnz, int n_docs, const uint16_t* __restrict__ q_dense,
    const uint16_t* __restrict__ d_dense, int dim, float w_dense, float w_lex, float* __restrict__ ws, int64_t stride) {
    constexpr int QP = HybPass<QCAP>::queries;
    __shared__ int32_t qt[QP * QCAP];
    __shared__ float qw[QP * QCAP];
    __shared__ uint32_t qd[QP * DC * 64];
    __shared__ int qn[QP];
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int chunks = dim >> 7, row_words = dim >> 1;
    // n_q <= QP: the queries of this pass (the host loops over passes)
    for (int q = 0; q < n_q; ++q) {
        const int nq = min(min(max(q_nnz[q], 0), kMaxQueryNnz), QCAP);   // (QCAP: max_q_nnz_host promised no more)
        const int qs = q_start[q];
        for (int i = threadIdx.x; i < nq; i += 64 * kHybWaves) {
            qt[q * QCAP + i] = q_terms[qs + i];
            qw[q * QCAP + i] = q_weights[qs + i];
        }
        for (int i = threadIdx.x; i < row_words; i += 64 * kHybWaves)
            qd[q * DC * 64 + i] = reinterpret_cast<const uint32_t*>(q_dense + (size_t)q * dim)[i];
        if (threadIdx.x == 0) qn[q] = nq;
    }
    __syncthreads();

    // lane kHybRun * q + r keeps the sums of (query q, document r of the run)
    const int my_q = lane / kHybRun, my_r = lane % kHybRun;
    const int64_t n_runs = ((int64_t)n_docs + kHybRun - 1) / kHybRun, n_waves = (int64_t)gridDim.x * kHybWaves;
    // a run's lengths and starts are fetched one step of the walk ahead: the loads of its rows and entries then wait for nothing
    int dn_next[kHybRun];
    int64_t ds_next[kHybRun];
    auto fetch_head = [&](int64_t run) {
#pragma unroll
        for (int r = 0; r < kHybRun; ++r) {
            const int64_t doc = run * kHybRun + r;
            const bool in = run < n_runs && doc < n_docs;
            dn_next[r] = in ? d_nnz[doc] : -1;
            ds_next[r] = in ? d_start[doc] : 0;
        }
    };
    int64_t run = (int64_t)blockIdx.x * kHybWaves + wave;
    fetch_head(run);
    for (; run < n_runs; run += n_waves) {   // (wave-uniform)
        const int doc0 = (int)(run * kHybRun);
        int dn[kHybRun];
        int64_t ds[kHybRun];
        int32_t dt[kHybRun][kHybRegs];
        float dw[kHybRun][kHybRegs];
        f32x2 dd[kHybRun][DC];
#pragma unroll
        for (int r = 0; r < kHybRun; ++r) {
            // (< 0: a tombstone, or behind the last document -- neither is read; the same value in every lane)
            dn[r] = __builtin_amdgcn_readfirstlane(min(dn_next[r], kMaxDocNnz));
            ds[r] = ds_next[r];
#pragma unroll
            for (int e = 0; e < kHybRegs; ++e) {
                dt[r][e] = 0;
                dw[r][e] = 0.f;
            }
#pragma unroll
            for (int c = 0; c < DC; ++c) dd[r][c] = f32x2{0.f, 0.f};
            if (dn[r] >= 0) {   // (wave-uniform)
                const int doc = doc0 + r;
#pragma unroll
                for (int c = 0; c < DC; ++c)
                    if (c < chunks) dd[r][c] = load_pair<false>(d_dense, (size_t)doc * dim + 128 * c + 2 * lane);
#pragma unroll
                for (int e = 0; e < kHybRegs; ++e) {
                    if (lane + 64 * e < dn[r]) {
                        dt[r][e] = d_terms[ds[r] + lane + 64 * e];
                        dw[r][e] = d_weights[ds[r] + lane + 64 * e];
                    }
                }
            }
        }
        fetch_head(run + n_waves);
        float my_lex = 0.f, my_dense = 0.f;
        bool my_live = false;
#pragma unroll
        for (int r = 0; r < kHybRun; ++r) {
            if (dn[r] < 0) continue;   // (wave-uniform)
            if (my_r == r) my_live = true;
            const int n_e = min((dn[r] + 63) >> 6, kHybRegs);   // register entries per lane this document uses (wave-uniform)
            for (int q = 0; q < n_q; ++q) {
                const int nq = __builtin_amdgcn_readfirstlane(qn[q]);
                const int32_t* qtq = qt + q * QCAP;
                const float* qwq = qw + q * QCAP;
                // lexical_score_kernel's bisection for each of the lane's register entries, the n_e of them side by side: a range of
                // nq halves to nothing in floor(log2 nq) + 1 steps, and a finished one stands still
                int lo[kHybRegs], hi[kHybRegs];
#pragma unroll
                for (int e = 0; e < kHybRegs; ++e) {
                    lo[e] = 0;
                    hi[e] = lane + 64 * e < dn[r] ? nq : 0;
                }
                for (int s = nq; s > 0; s >>= 1) {
#pragma unroll
                    for (int e = 0; e < kHybRegs; ++e) {
                        if (e < n_e) {
                            const bool on = lo[e] < hi[e];
                            const int mid = (lo[e] + hi[e]) >> 1;
                            const bool less = qtq[on ? mid : 0] < dt[r][e];
                            lo[e] = on && less ? mid + 1 : lo[e];
                            hi[e] = on && !less ? mid : hi[e];
                        }
                    }
                }
                float acc = 0.f;
#pragma unroll
                for (int e = 0; e < kHybRegs; ++e) {   // (entries lane, lane + 64, ... in that order)
                    if (e < n_e) {
                        const bool in = lane + 64 * e < dn[r] && lo[e] < nq;
                        const int at = in ? lo[e] : 0;
                        if (in && qtq[at] == dt[r][e]) acc = fmaf(qwq[at], dw[r][e], acc);
                    }
                }
                for (int j = lane + 64 * kHybRegs; j < dn[r]; j += 64) acc = hybrid_match(qtq, qwq, nq, d_terms[ds[r] + j], d_weights + ds[r] + j, acc);
                const float lex = wave_sum(acc);
                const uint32_t* qdq = qd + q * DC * 64 + lane;
                float dacc = 0.f;
#pragma unroll
                for (int c = 0; c < DC; ++c) {
                    if (c < chunks) {
                        const uint32_t u = qdq[64 * c];
                        dacc = fmaf(elo(u), dd[r][c].x, dacc);
                        dacc = fmaf(ehi(u), dd[r][c].y, dacc);
                    }
                }
                const float dense = wave_sum(dacc);
                if (lane == kHybRun * q + r) {
                    my_lex = lex;
                    my_dense = dense;
                }
            }
        }
        if (my_q < n_q && doc0 + my_r < n_docs)
            ws[(size_t)my_q * stride + doc0 + my_r] = my_live ? hybrid_mix(w_dense, my_dense, w_lex, my_lex) : __builtin_nanf("");
    }
}

__global__ void lexical_pad_kernel(float* s, int32_t* ix, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) {
        s[i] = -INFINITY;
        ix[i] = -1;
    }
}

// `grid_cand`: how many candidates the grid is sized for (the walk is grid-strided, so any value >= 1 scores every pair)
int score_launch(const int32_t* q_terms, const float* q_weights, const int32_t* q_start, const int32_t* q_nnz, int n_q,
                 const int32_t* d_terms, const float* d_weights, const int64_t* d_start, const int32_t* d_nnz, const int32_t* cand,
                 const int32_t* cand_cnt, int64_t cand_stride, int grid_cand, int n_cand, int64_t out_stride, const void* q_dense,
                 const void* d_dense, int dim, float w_dense, float w_lex, float dead, float* out_lex, float* out_dense,
                 float* out_hybrid, hipStream_t st) {
    const int groups = (std::max(std::min(grid_cand, n_cand), 1) + kScoreWaves - 1) / kScoreWaves;
    // enough workgroups to fill every CU several times over; a wave walks the candidates behind its first one
    const dim3 grid((unsigned)std::min(groups, 8192), (unsigned)n_q);
    TtProfScope prof(TT_K_ROWOPS, st);
    hipLaunchKernelGGL(lexical_score_kernel, grid, dim3(64 * kScoreWaves), 0, st, q_terms, q_weights, q_start, q_nnz, d_terms,
                       d_weights, d_start, d_nnz, cand, cand_cnt, cand_stride, n_cand, out_stride, (const uint16_t*)q_dense,
                       (const uint16_t*)d_dense, dim, w_dense, w_lex, dead, out_lex, out_dense, out_hybrid);
    TT_CHECK_LAUNCH();
    return TT_OK;
}
#endif  // !TT_F16

template <bool F32>
int weights_launch(const char* name, const void* hidden, int n_rows, int ld, int H, const void* w, float bias, const int32_t* ids,
                   const int32_t* seq_start, const int32_t* seq_len, int n_seq, int max_len, int skip0, int skip1, int skip2, int skip3,
                   int32_t* out_terms, float* out_weights, int32_t* out_nnz, hipStream_t st) {
    if (H <= 0 || H % 128 || H > kMaxH) {
        tt_set_error("%s: hidden=%d must be a multiple of 128 and <= %d", name, H, kMaxH);
        return TT_E_UNSUPPORTED;
    }
    if (max_len <= 0 || max_len > kMaxSeqLen) {
        tt_set_error("%s: max_len=%d (sequences of 1 .. %d rows)", name, max_len, kMaxSeqLen);
        return TT_E_UNSUPPORTED;
    }
    TT_CHECK_ARG(n_seq >= 0 && n_seq <= 65535 && n_rows >= 0 && ld >= H && ld % 2 == 0, "n_seq=%d n_rows=%d ld=%d hidden=%d", n_seq,
                 n_rows, ld, H);
    if (n_seq == 0) return TT_OK;
    TT_CHECK_ARG(hidden && w && ids && seq_start && seq_len && out_terms && out_weights && out_nnz, "null pointer");
    // the instantiation whose LDS image holds max_len pairs: a batch of 64-token queries does not pay for 8192
    const int cap = max_len <= 64 ? 64 : (max_len <= 512 ? 512 : (max_len <= 2048 ? 2048 : kMaxSeqLen));
    const Skip4 skip{skip0, skip1, skip2, skip3};
    TtProfScope prof(TT_K_ROWOPS, st);
    hipLaunchKernelGGL(lexical_dot_kernel<F32>, dim3((max_len + kDotRows - 1) / kDotRows, n_seq), dim3(64 * kDotWaves), 0, st, hidden, ld,
                       H, w, bias, seq_start, seq_len, cap, n_rows, out_weights);
    TT_CHECK_LAUNCH();
#define TT_LEX_DEDUP(N)                                                                                                           \
    hipLaunchKernelGGL(lexical_dedup_kernel<N>, dim3(n_seq), dim3(DedupShape<N>::threads), 0, st, ids, seq_start, seq_len, n_rows,   \
                       skip, out_terms, out_weights, out_nnz)
    switch (cap) {
        case 64: TT_LEX_DEDUP(64); break;
        case 512: TT_LEX_DEDUP(512); break;
        case 2048: TT_LEX_DEDUP(2048); break;
        default: TT_LEX_DEDUP(kMaxSeqLen); break;
    }
#undef TT_LEX_DEDUP
    TT_CHECK_LAUNCH();
    return TT_OK;
}

}  // namespace

extern "C" {

int tt_lexical_weights(const void* hidden, int n_rows, int ld, int H, const void* w, float bias_host, const int32_t* ids,
                       const int32_t* seq_start, const int32_t* seq_len, int n_seq, int max_len, int skip0_host, int skip1_host,
                       int skip2_host, int skip3_host, int32_t* out_terms, float* out_weights, int32_t* out_nnz, void* stream) {
    return weights_launch<false>(kF16 ? "tt_lexical_weights_f16" : "tt_lexical_weights", hidden, n_rows, ld, H, w, bias_host, ids, seq_start, seq_len, n_seq, max_len,
                                 skip0_host, skip1_host, skip2_host, skip3_host, out_terms, out_weights, out_nnz, (hipStream_t)stream);
}

#if !TT_F16
int tt_lexical_weights_f32(const float* hidden, int n_rows, int ld, int H, const float* w, float bias_host, const int32_t* ids,
                           const int32_t* seq_start, const int32_t* seq_len, int n_seq, int max_len, int skip0_host, int skip1_host,
                           int skip2_host, int skip3_host, int32_t* out_terms, float* out_weights, int32_t* out_nnz, void* stream) {
    return weights_launch<true>("tt_lexical_weights_f32", hidden, n_rows, ld, H, w, bias_host, ids, seq_start, seq_len, n_seq, max_len,
                                skip0_host, skip1_host, skip2_host, skip3_host, out_terms, out_weights, out_nnz, (hipStream_t)stream);
}

static int check_score_args(const char* name, const void* q_terms, const void* q_weights, const void* q_start, const void* q_nnz,
                            int n_q, const void* d_terms, const void* d_weights, const void* d_start, const void* d_nnz,
                            const void* q_dense, const void* d_dense, int dim, float w_dense, float w_lex) {
    TT_CHECK_ARG(n_q >= 0 && n_q <= 65535, "%s: n_q=%d", name, n_q);
    TT_CHECK_ARG(q_terms && q_weights && q_start && q_nnz && d_terms && d_weights && d_start && d_nnz, "%s: null pointer", name);
    if (q_dense) {
        TT_CHECK_ARG(d_dense != nullptr, "%s: q_dense without d_dense", name);
        if (dim <= 0 || dim % 128 || dim > kMaxH) {
            tt_set_error("%s: dim=%d must be a multiple of 128 and <= %d", name, dim, kMaxH);
            return TT_E_UNSUPPORTED;
        }
        TT_CHECK_ARG(w_dense >= 0.f && w_lex >= 0.f && w_dense + w_lex > 0.f, "%s: w_dense=%g w_lex=%g (both >= 0, not both 0)", name,
                     (double)w_dense, (double)w_lex);
    }
    return TT_OK;
}

int tt_lexical_score(const int32_t* q_terms, const float* q_weights, const int32_t* q_start, const int32_t* q_nnz, int n_q,
                     const int32_t* d_terms, const float* d_weights, const int64_t* d_start, const int32_t* d_nnz, const int32_t* cand,
                     int n_cand, const void* q_dense, const void* d_dense, int dim, float w_dense, float w_lex, float* out_lex,
                     float* out_dense, float* out_hybrid, void* stream) {
    TT_CHECK_ARG(n_cand >= 0, "tt_lexical_score: n_cand=%d", n_cand);
    if (n_q == 0 || n_cand == 0) return TT_OK;
    int rc = check_score_args("tt_lexical_score", q_terms, q_weights, q_start, q_nnz, n_q, d_terms, d_weights, d_start, d_nnz, q_dense,
                              d_dense, dim, w_dense, w_lex);
    if (rc) return rc;
    TT_CHECK_ARG(out_lex && (!q_dense || (out_dense && out_hybrid)), "tt_lexical_score: null output");
    return score_launch(q_terms, q_weights, q_start, q_nnz, n_q, d_terms, d_weights, d_start, d_nnz, cand, nullptr, n_cand, n_cand,
                        n_cand, n_cand, q_dense, d_dense, dim, w_dense, w_lex, -INFINITY, out_lex, out_dense, out_hybrid,
                        (hipStream_t)stream);
}

size_t tt_lexical_scan_workspace_bytes(int64_t n_docs, int n_q) {
    if (n_docs < 0 || n_q <= 0) return 0;
    const int64_t stride = (n_docs + 31) / 32 * 32;
    return tt_align_up((size_t)n_q * stride * sizeof(float), 256);
}

int tt_lexical_scan_topk(const int32_t* q_terms, const float* q_weights, const int32_t* q_start, const int32_t* q_nnz, int n_q,
                         const int32_t* d_terms, const float* d_weights, const int64_t* d_start, const int32_t* d_nnz, int64_t n_docs,
                         int k, float* out_scores, int32_t* out_idx, void* workspace, size_t workspace_bytes, void* stream) {
    if (n_q < 1 || n_q > 64 || k < 1 || k > 1024) {
        tt_set_error("tt_lexical_scan_topk: n_q=%d (1 .. 64), k=%d (1 .. 1024)", n_q, k);
        return TT_E_UNSUPPORTED;
    }
    TT_CHECK_ARG(n_docs >= 0 && n_docs <= INT_MAX, "tt_lexical_scan_topk: n_docs=%lld", (long long)n_docs);
    TT_CHECK_ARG(out_scores && out_idx, "tt_lexical_scan_topk: null output");
    hipStream_t st = (hipStream_t)stream;
    if (n_docs == 0) {
        const int64_t n = (int64_t)n_q * k;
        hipLaunchKernelGGL(lexical_pad_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, out_scores, out_idx, n);
        TT_CHECK_LAUNCH();
        return TT_OK;
    }
    int rc = check_score_args("tt_lexical_scan_topk", q_terms, q_weights, q_start, q_nnz, n_q, d_terms, d_weights, d_start, d_nnz,
                              nullptr, nullptr, 0, 0.f, 0.f);
    if (rc) return rc;
    const size_t need = tt_lexical_scan_workspace_bytes(n_docs, n_q);
    if (!workspace || workspace_bytes < need) {
        tt_set_error("tt_lexical_scan_topk: workspace %zu < required %zu bytes", workspace_bytes, need);
        return TT_E_WORKSPACE;
    }
    const int64_t stride = (n_docs + 31) / 32 * 32;
    float* dense = (float*)workspace;
    // a tombstone's slot holds NaN, what a deleted row of the dense index scores (vector_index.py): the selection's key rejects it
    rc = score_launch(q_terms, q_weights, q_start, q_nnz, n_q, d_terms, d_weights, d_start, d_nnz, nullptr, nullptr, 0, (int)n_docs,
                      (int)n_docs, stride, nullptr, nullptr, 0, 0.f, 0.f, __builtin_nanf(""), dense, nullptr, nullptr, st);
    if (rc) return rc;
    SelectParams se{};
    se.scores = dense;
    se.idx = nullptr;
    se.stride = stride;
    se.cnt = nullptr;
    se.m_fixed = (int)n_docs;
    se.cap = INT_MAX;
    se.idx_base = 0;
    se.k = k;
    se.out_scores = out_scores;
    se.out_idx = out_idx;
    se.out_stride = k;
    return tt_select_launch(se, n_q, st);
}

size_t tt_hybrid_scan_workspace_bytes(int64_t n_docs, int n_q) { return tt_lexical_scan_workspace_bytes(n_docs, n_q); }

int tt_hybrid_scan_topk(const int32_t* q_terms, const float* q_weights, const int32_t* q_start, const int32_t* q_nnz, int n_q,
                        int max_q_nnz_host, const int32_t* d_terms, const float* d_weights, const int64_t* d_start,
                        const int32_t* d_nnz, int64_t n_docs, const void* q_dense, const void* d_dense, int dim, float w_dense,
                        float w_lex, int k, float* out_scores, int32_t* out_idx, void* workspace, size_t workspace_bytes,
                        void* stream) {
    const char* name = "tt_hybrid_scan_topk";
    if (dim <= 0 || dim % 128 || dim > kMaxH) {
        tt_set_error("%s: dim=%d must be a multiple of 128 and <= %d", name, dim, kMaxH);
        return TT_E_UNSUPPORTED;
    }
    if (n_q < 1 || n_q > 64 || k < 1 || k > 1024 || max_q_nnz_host < 0 || max_q_nnz_host > kMaxQueryNnz) {
        tt_set_error("%s: n_q=%d (1 .. 64), k=%d (1 .. 1024), max_q_nnz=%d (0 .. %d)", name, n_q, k, max_q_nnz_host, kMaxQueryNnz);
        return TT_E_UNSUPPORTED;
    }
    TT_CHECK_ARG(n_docs >= 0 && n_docs <= INT_MAX, "%s: n_docs=%lld", name, (long long)n_docs);
    TT_CHECK_ARG(out_scores && out_idx, "%s: null output", name);
    TT_CHECK_ARG(w_dense >= 0.f && w_lex >= 0.f && w_dense + w_lex > 0.f, "%s: w_dense=%g w_lex=%g (both >= 0, not both 0)", name,
                 (double)w_dense, (double)w_lex);
    hipStream_t st = (hipStream_t)stream;
    if (n_docs == 0) {   // (an empty store's arrays may be null)
        const int64_t n = (int64_t)n_q * k;
        hipLaunchKernelGGL(lexical_pad_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, out_scores, out_idx, n);
        TT_CHECK_LAUNCH();
        return TT_OK;
    }
    TT_CHECK_ARG(q_dense && d_dense, "%s: null dense vectors", name);
    int rc = check_score_args(name, q_terms, q_weights, q_start, q_nnz, n_q, d_terms, d_weights, d_start, d_nnz, q_dense, d_dense,
                              dim, w_dense, w_lex);
    if (rc) return rc;
    const size_t need = tt_hybrid_scan_workspace_bytes(n_docs, n_q);
    if (!workspace || workspace_bytes < need) {
        tt_set_error("%s: workspace %zu < required %zu bytes", name, workspace_bytes, need);
        return TT_E_WORKSPACE;
    }
    const int cus = tt_cu_count_cached();
    TT_CHECK_ARG(cus > 0, "%s: no device", name);
    const int64_t stride = (n_docs + 31) / 32 * 32;
    float* dense = (float*)workspace;
    // a persistent grid: kHybWgPerCu workgroups per compute unit, never more than there are runs for their waves
    const int64_t runs = (n_docs + kHybRun - 1) / kHybRun;
    const int grid = (int)std::min<int64_t>((int64_t)cus * kHybWgPerCu, (runs + kHybWaves - 1) / kHybWaves);
    const bool shrt = max_q_nnz_host <= kHybShort;
    const int per_pass = shrt ? HybPass<kHybShort>::queries : HybPass<kMaxQueryNnz>::queries;
    const uint16_t* qd = (const uint16_t*)q_dense;
    {
        TtProfScope prof(TT_K_ROWOPS, st);
        // one sweep of the store per pass, into the pass's own workspace rows: a score does not know which pass it is in
        for (int q_lo = 0; q_lo < n_q; q_lo += per_pass) {
            const int n_pass = std::min(per_pass, n_q - q_lo);
#define TT_HYBRID_SCAN(DC, QCAP)                                                                                                   \
    hipLaunchKernelGGL((hybrid_scan_kernel<DC, QCAP>), dim3(grid), dim3(64 * kHybWaves), 0, st, q_terms, q_weights, q_start + q_lo,    \
                       q_nnz + q_lo, n_pass, d_terms, d_weights, d_start, d_nnz, (int)n_docs, qd + (size_t)q_lo * dim,               \
                       (const uint16_t*)d_dense, dim, w_dense, w_lex, dense + (size_t)q_lo * stride, stride)
            if (dim <= 256) {
                if (shrt) TT_HYBRID_SCAN(2, kHybShort); else TT_HYBRID_SCAN(2, kMaxQueryNnz);
            } else if (dim <= 512) {
                if (shrt) TT_HYBRID_SCAN(4, kHybShort); else TT_HYBRID_SCAN(4, kMaxQueryNnz);
            } else {
                if (shrt) TT_HYBRID_SCAN(8, kHybShort); else TT_HYBRID_SCAN(8, kMaxQueryNnz);
            }
#undef TT_HYBRID_SCAN
            TT_CHECK_LAUNCH();
        }
    }
    // the lexical scan's selection: a tombstone's slot holds NaN, which the selection's key rejects
    SelectParams se{};
    se.scores = dense;
    se.idx = nullptr;
    se.stride = stride;
    se.cnt = nullptr;
    se.m_fixed = (int)n_docs;
    se.cap = INT_MAX;
    se.idx_base = 0;
    se.k = k;
    se.out_scores = out_scores;
    se.out_idx = out_idx;
    se.out_stride = k;
    return tt_select_launch(se, n_q, st);
}
#endif  // !TT_F16

}  // extern "C"

#if !TT_F16
// scan.h: the lexical scores of per-query candidate lists for postings.hip -- lexical_score_kernel as tt_lexical_scan_topk launches
// it (no dense part, `dead` for a tombstone), over cand[q * stride .. + min(cand_cnt[q], stride)), scores at the same positions
int tt_lexical_score_lists(const int32_t* q_terms, const float* q_weights, const int32_t* q_start, const int32_t* q_nnz, int n_q,
                           const int32_t* d_terms, const float* d_weights, const int64_t* d_start, const int32_t* d_nnz,
                           const int32_t* cand, const int32_t* cand_cnt, int64_t stride, int grid_cand, float dead, float* out_lex,
                           hipStream_t st) {
    return score_launch(q_terms, q_weights, q_start, q_nnz, n_q, d_terms, d_weights, d_start, d_nnz, cand, cand_cnt, stride, grid_cand,
                        (int)stride, stride, nullptr, nullptr, 0, 0.f, 0.f, dead, out_lex, nullptr, nullptr, st);
}
#endif
