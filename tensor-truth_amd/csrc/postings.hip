// Posting lists for the lexical / SPLADE stores (include/tt_hip.h, "Posting lists: an exact candidate generator").
//   tt_postings_build          forward index (the stores' CSR arrays) -> per-term document lists, per-term maximum weight, flag word
//   tt_lexical_topk_postings   the union of a query's chosen lists (+ the unsealed tail) as an ascending candidate list, scored by
//                              lexical_score_kernel (lexical.hip) and selected by select.hip: tt_lexical_scan_topk's bits over the
//                              candidates instead of over every document
// The lists only CHOOSE candidates; a score is computed by the scan's own kernel and a result picked by the scan's own selection, so
// whatever both paths return for a document is the same bits.  When the candidates hold the whole top-k is the host's decision
// (postings.py: thr_out > 0, MaxScore bounds), not this file's.
//
// Atomics: integer atomicAdd / atomicOr only, none of which decides where a candidate is written -- the fill order inside one list
// is unspecified by contract, a bitmap bit is idempotent, and the compaction takes its positions from popcounts and scans.  The
// flag word gets one atomicOr per wave.
#include "common.h"
#include "scan.h"

#include <limits.h>

#include <algorithm>

namespace {

constexpr int kMaxDocNnz = 8192;        // lexical_score_kernel's clamp of d_nnz: entries behind it are neither scored nor indexed
constexpr int kWalkWaves = 4;           // waves of a forward-index workgroup: one document per wave
constexpr int kScanThreads = 1024;      // the single-workgroup exclusive scans
constexpr int kSpanThreads = 256;       // a compaction workgroup: one bitmap word per thread ...
constexpr int kSpanWords = kSpanThreads;
constexpr int kSpan = 32 * kSpanWords;  // ... so 8192 documents per workgroup (TT_POSTINGS_SPAN)
static_assert(kSpan == TT_POSTINGS_SPAN, "tt_hip.h names the compaction span");

// ---- build --------------------------------------------------------------------------------------------------------------------------
// One wave per document of [0, n_sealed), lane l its entries l, l + 64, ... (lexical_score_kernel's walk).  A tombstone is skipped.
//   MODE 0  histogram: cnt[term] += 1; flag 1 for a term outside [0, vocab), flag 2 for a weight that is negative, NaN or infinite,
//           flag 4 for a document whose ids are not strictly ascending (a repeated id among them)
//   MODE 1  fill: slot = post_off[term] + (--cnt[term]) -- the histogram's counts run back down to 0, so every slot of a list is
//           taken once and none beside it; a slot at or behind post_cap is not written whatever the counters say
//   MODE 2  per-term maximum over the finite weights >= 0 (a non-negative float's bits order as the float does: integer atomicMax)
template <int MODE>
__global__ __launch_bounds__(64 * kWalkWaves) void postings_walk_kernel(const int32_t* __restrict__ d_terms,
                                                                        const float* __restrict__ d_weights,
                                                                        const int64_t* __restrict__ d_start,
                                                                        const int32_t* __restrict__ d_nnz, int64_t n_sealed, int vocab,
                                                                        uint32_t* __restrict__ cnt, const int64_t* __restrict__ post_off,
                                                                        int32_t* __restrict__ post_doc, int64_t post_cap,
                                                                        uint32_t* __restrict__ term_ub_bits, int32_t* __restrict__ flags) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int bad = 0;
    for (int64_t doc = (int64_t)blockIdx.x * kWalkWaves + wave; doc < n_sealed; doc += (int64_t)gridDim.x * kWalkWaves) {   // (wave-uniform)
        const int dn_raw = d_nnz[doc];
        if (dn_raw < 0) continue;
        const int dn = min(dn_raw, kMaxDocNnz);
        const int64_t ds = d_start[doc];
        for (int j = lane; j < dn; j += 64) {
            const int32_t t = d_terms[ds + j];
            const bool in_vocab = (uint32_t)t < (uint32_t)vocab;
            if constexpr (MODE == 0) {
                const float w = d_weights[ds + j];
                if (!in_vocab) bad |= 1;
                else atomicAdd(&cnt[t], 1u);
                if (!(w >= 0.f && w < INFINITY)) bad |= 2;
                // tt_lexical_score's precondition, ascending and distinct ids: a repeated id is added once per occurrence by the
                // scoring kernel, so a per-term maximum would not bound what it contributes
                if (j > 0 && d_terms[ds + j - 1] >= t) bad |= 4;
            } else if constexpr (MODE == 1) {
                if (in_vocab) {
                    const uint32_t before = atomicSub(&cnt[t], 1u);
                    const int64_t slot = post_off[t] + (int64_t)before - 1;
                    if (before != 0u && before <= 0x7FFFFFFFu && slot >= 0 && slot < post_cap) post_doc[slot] = (int32_t)doc;
                }
            } else {
                const float w = d_weights[ds + j];
                if (in_vocab && w > 0.f && w < INFINITY) atomicMax(&term_ub_bits[t], __float_as_uint(w));
            }
        }
    }
    if constexpr (MODE == 0) {
        const int any = (__builtin_amdgcn_ballot_w64((bad & 1) != 0) ? 1 : 0) | (__builtin_amdgcn_ballot_w64((bad & 2) != 0) ? 2 : 0) |
                        (__builtin_amdgcn_ballot_w64((bad & 4) != 0) ? 4 : 0);
        if (any && lane == 0) atomicOr(flags, any);
    }
}

// Exclusive scan of n values by one workgroup: thread t sums the values [t * per, (t + 1) * per), the 1024 sums are scanned in LDS,
// and the thread writes its values' prefixes.  out[n] = the total.  In place when IN and OUT are one type and one array.
template <typename IN, typename OUT>
__global__ __launch_bounds__(kScanThreads) void postings_scan_kernel(const IN* in, int64_t n, int64_t in_stride, OUT* out,
                                                                     int64_t out_stride, int32_t* total_plus, int32_t plus) {
    __shared__ long long sums[2][kScanThreads];
    const int tid = threadIdx.x;
    in += (int64_t)blockIdx.x * in_stride;
    out += (int64_t)blockIdx.x * out_stride;
    const int64_t per = (n + kScanThreads - 1) / kScanThreads;
    const int64_t i0 = (int64_t)tid * per < n ? (int64_t)tid * per : n, i1 = i0 + per < n ? i0 + per : n;
    long long mine = 0;
    for (int64_t i = i0; i < i1; ++i) mine += (long long)in[i];
    sums[0][tid] = mine;
    __syncthreads();
    int cur = 0;
    for (int off = 1; off < kScanThreads; off <<= 1) {   // inclusive prefix sums
        const long long v = sums[cur][tid] + (tid >= off ? sums[cur][tid - off] : 0);
        sums[cur ^ 1][tid] = v;
        cur ^= 1;
        __syncthreads();
    }
    long long run = sums[cur][tid] - mine;
    for (int64_t i = i0; i < i1; ++i) {
        const long long v = (long long)in[i];   // (read before the slot is overwritten: in place)
        out[i] = (OUT)run;
        run += v;
    }
    if (tid == kScanThreads - 1) {
        out[n] = (OUT)sums[cur][tid];
        if (total_plus) total_plus[blockIdx.x] = (int32_t)sums[cur][tid] + plus;
    }
}

// ---- candidates ---------------------------------------------------------------------------------------------------------------------
// Query q ORs the documents of its ranges r in [range_start[q], range_start[q + 1]) -- post_doc[range_lo[r] .. range_hi[r]), cut to
// [0, post_len) -- into its bitmap.  A document number outside [0, n_sealed) sets nothing.  A bit that already reads as set is not
// ORed again (lists of one query overlap; a stale read only costs the atomic it would have saved).
__global__ __launch_bounds__(256) void postings_mark_kernel(const int32_t* __restrict__ post_doc, int64_t post_len,
                                                            const int64_t* __restrict__ range_lo, const int64_t* __restrict__ range_hi,
                                                            const int32_t* __restrict__ range_start, int64_t n_sealed,
                                                            uint32_t* __restrict__ bitmap, int64_t words_q) {
    const int q = blockIdx.y;
    uint32_t* bm = bitmap + (int64_t)q * words_q;
    const int r1 = range_start[q + 1];
    for (int r = range_start[q]; r < r1; ++r) {
        const int64_t rl = range_lo[r], rh = range_hi[r];
        const int64_t lo = rl > 0 ? rl : 0, hi = rh < post_len ? rh : post_len;
        for (int64_t i = lo + (int64_t)blockIdx.x * 256 + threadIdx.x; i < hi; i += (int64_t)gridDim.x * 256) {
            const int32_t d = post_doc[i];
            if (d >= 0 && (int64_t)d < n_sealed) {
                const uint32_t bit = 1u << (d & 31);
                uint32_t* w = bm + (d >> 5);
                if (!(__atomic_load_n(w, __ATOMIC_RELAXED) & bit)) atomicOr(w, bit);
            }
        }
    }
}

// blk[q][b] = set bits of the 256 words of span b
__global__ __launch_bounds__(kSpanThreads) void postings_count_kernel(const uint32_t* __restrict__ bitmap, int64_t words_q, int nb,
                                                                      int32_t* __restrict__ blk) {
    __shared__ int part[kSpanThreads / 64];
    const int q = blockIdx.y, b = blockIdx.x, tid = threadIdx.x;
    int c = __popc(bitmap[(int64_t)q * words_q + (int64_t)b * kSpanWords + tid]);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o, 64);
    if ((tid & 63) == 0) part[tid >> 6] = c;
    __syncthreads();
    if (tid == 0) blk[(int64_t)q * (nb + 1) + b] = part[0] + part[1] + part[2] + part[3];
}

// span b of query q writes its set bits, ascending, from position blk[q][b] (now the exclusive scan) on
__global__ __launch_bounds__(kSpanThreads) void postings_write_kernel(const uint32_t* __restrict__ bitmap, int64_t words_q, int nb,
                                                                      const int32_t* __restrict__ blk, int32_t* __restrict__ cand,
                                                                      int64_t stride) {
    __shared__ int pre[2][kSpanThreads];
    const int q = blockIdx.y, b = blockIdx.x, tid = threadIdx.x;
    uint32_t word = bitmap[(int64_t)q * words_q + (int64_t)b * kSpanWords + tid];
    const int mine = __popc(word);
    pre[0][tid] = mine;
    __syncthreads();
    int cur = 0;
    for (int off = 1; off < kSpanThreads; off <<= 1) {   // inclusive prefix sums
        const int v = pre[cur][tid] + (tid >= off ? pre[cur][tid - off] : 0);
        pre[cur ^ 1][tid] = v;
        cur ^= 1;
        __syncthreads();
    }
    int64_t pos = (int64_t)blk[(int64_t)q * (nb + 1) + b] + pre[cur][tid] - mine;
    const int32_t doc0 = (b * kSpanWords + tid) * 32;
    int32_t* out = cand + (int64_t)q * stride;
    while (word) {
        if (pos < stride) out[pos] = doc0 + __builtin_ctz(word);   // (always: at most n_sealed <= stride bits are set)
        ++pos;
        word &= word - 1;
    }
}

// the unsealed tail, whole, behind query q's blk[q][nb] listed documents
__global__ __launch_bounds__(256) void postings_tail_kernel(const int32_t* __restrict__ blk, int nb, int64_t n_sealed, int64_t n_docs,
                                                            int32_t* __restrict__ cand, int64_t stride) {
    const int q = blockIdx.y;
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t pos = (int64_t)blk[(int64_t)q * (nb + 1) + nb] + i;
    if (n_sealed + i < n_docs && pos < stride) cand[(int64_t)q * stride + pos] = (int32_t)(n_sealed + i);
}

__global__ void postings_pad_kernel(float* s, int32_t* ix, int64_t n, float* thr, int32_t* cnt, int32_t* cand_cnt, int n_q) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) {
        s[i] = -INFINITY;
        ix[i] = -1;
    }
    if (i < n_q) {
        if (thr) thr[i] = -INFINITY;
        if (cnt) cnt[i] = 0;
        if (cand_cnt) cand_cnt[i] = 0;
    }
}

struct Layout {
    int nb;
    int64_t words_q, stride;
    size_t off_blk, off_cand, off_scores, total;
};

Layout layout_of(int64_t n_docs, int64_t n_sealed, int n_q) {
    Layout l{};
    l.nb = (int)((n_sealed + kSpan - 1) / kSpan);
    l.words_q = (int64_t)l.nb * kSpanWords;
    l.stride = (n_docs + 31) / 32 * 32;
    size_t at = tt_align_up((size_t)n_q * l.words_q * sizeof(uint32_t), 256);
    l.off_blk = at;
    at += tt_align_up((size_t)n_q * (l.nb + 1) * sizeof(int32_t), 256);
    l.off_cand = at;
    at += tt_align_up((size_t)n_q * l.stride * sizeof(int32_t), 256);
    l.off_scores = at;
    at += tt_align_up((size_t)n_q * l.stride * sizeof(float), 256);
    l.total = at;
    return l;
}

}  // namespace

extern "C" {

size_t tt_postings_build_workspace_bytes(int vocab) {
    return vocab > 0 ? tt_align_up((size_t)vocab * sizeof(uint32_t), 256) : 0;
}

int tt_postings_build(const int32_t* d_terms, const float* d_weights, const int64_t* d_start, const int32_t* d_nnz, int64_t n_sealed,
                      int vocab, int64_t* post_off, int32_t* post_doc, int64_t post_cap, float* term_ub, int32_t* flags,
                      void* workspace, size_t workspace_bytes, void* stream) {
    TT_CHECK_ARG(vocab >= 1 && n_sealed >= 0 && n_sealed <= INT_MAX - 64 && post_cap >= 0, "tt_postings_build: vocab=%d n_sealed=%lld post_cap=%lld",
                 vocab, (long long)n_sealed, (long long)post_cap);
    TT_CHECK_ARG(post_off && term_ub && flags && (post_doc || post_cap == 0), "tt_postings_build: null output");
    TT_CHECK_ARG(n_sealed == 0 || (d_terms && d_weights && d_start && d_nnz), "tt_postings_build: null pointer");
    const size_t need = tt_postings_build_workspace_bytes(vocab);
    if (!workspace || workspace_bytes < need) {
        tt_set_error("tt_postings_build: workspace %zu < required %zu bytes", workspace_bytes, need);
        return TT_E_WORKSPACE;
    }
    hipStream_t st = (hipStream_t)stream;
    uint32_t* cnt = (uint32_t*)workspace;
    TT_CHECK_HIP(hipMemsetAsync(cnt, 0, (size_t)vocab * sizeof(uint32_t), st));
    TT_CHECK_HIP(hipMemsetAsync(term_ub, 0, (size_t)vocab * sizeof(float), st));
    TT_CHECK_HIP(hipMemsetAsync(flags, 0, sizeof(int32_t), st));
    const dim3 grid((unsigned)std::min<int64_t>((n_sealed + kWalkWaves - 1) / kWalkWaves, 16384)), block(64 * kWalkWaves);
    TtProfScope prof(TT_K_ROWOPS, st);
    if (n_sealed > 0) {
        hipLaunchKernelGGL(postings_walk_kernel<0>, grid, block, 0, st, d_terms, d_weights, d_start, d_nnz, n_sealed, vocab, cnt,
                           (const int64_t*)nullptr, (int32_t*)nullptr, (int64_t)0, (uint32_t*)nullptr, flags);
        TT_CHECK_LAUNCH();
    }
    hipLaunchKernelGGL((postings_scan_kernel<uint32_t, int64_t>), dim3(1), dim3(kScanThreads), 0, st, cnt, (int64_t)vocab, (int64_t)0,
                       post_off, (int64_t)0, (int32_t*)nullptr, 0);
    TT_CHECK_LAUNCH();
    // the one readback of the build: an out-of-range term, or more entries than post_doc holds, ends it before anything is filled
    int32_t flags_host = 0;
    int64_t total_host = 0;
    TT_CHECK_HIP(hipMemcpyAsync(&flags_host, flags, sizeof(int32_t), hipMemcpyDeviceToHost, st));
    TT_CHECK_HIP(hipMemcpyAsync(&total_host, post_off + vocab, sizeof(int64_t), hipMemcpyDeviceToHost, st));
    TT_CHECK_HIP(hipStreamSynchronize(st));
    TT_CHECK_ARG(!(flags_host & 1), "tt_postings_build: a stored term lies outside the vocabulary [0, %d)", vocab);
    TT_CHECK_ARG(total_host <= post_cap, "tt_postings_build: %lld entries for post_doc of %lld", (long long)total_host, (long long)post_cap);
    if (n_sealed > 0) {
        hipLaunchKernelGGL(postings_walk_kernel<1>, grid, block, 0, st, d_terms, d_weights, d_start, d_nnz, n_sealed, vocab, cnt,
                           (const int64_t*)post_off, post_doc, post_cap, (uint32_t*)nullptr, (int32_t*)nullptr);
        TT_CHECK_LAUNCH();
        hipLaunchKernelGGL(postings_walk_kernel<2>, grid, block, 0, st, d_terms, d_weights, d_start, d_nnz, n_sealed, vocab,
                           (uint32_t*)nullptr, (const int64_t*)nullptr, (int32_t*)nullptr, (int64_t)0, (uint32_t*)term_ub,
                           (int32_t*)nullptr);
        TT_CHECK_LAUNCH();
    }
    return TT_OK;
}

size_t tt_lexical_topk_postings_workspace_bytes(int64_t n_docs, int64_t n_sealed, int n_q) {
    if (n_docs < 0 || n_sealed < 0 || n_sealed > n_docs || n_q <= 0 || n_docs > INT_MAX - 64) return 0;
    return layout_of(n_docs, n_sealed, n_q).total;
}

int tt_lexical_topk_postings(const int32_t* q_terms, const float* q_weights, const int32_t* q_start, const int32_t* q_nnz, int n_q,
                             const int32_t* d_terms, const float* d_weights, const int64_t* d_start, const int32_t* d_nnz, int64_t n_docs,
                             const int32_t* post_doc, int64_t post_len, int64_t n_sealed, const int64_t* range_lo,
                             const int64_t* range_hi, const int32_t* range_start, int64_t grid_entries, int k, float* out_scores,
                             int32_t* out_idx, float* thr_out, int32_t* cnt_out, int32_t* cand_cnt_out, void* workspace,
                             size_t workspace_bytes, void* stream) {
    if (n_q < 1 || n_q > 64 || k < 1 || k > 1024) {
        tt_set_error("tt_lexical_topk_postings: n_q=%d (1 .. 64), k=%d (1 .. 1024)", n_q, k);
        return TT_E_UNSUPPORTED;
    }
    TT_CHECK_ARG(n_docs >= 0 && n_docs <= INT_MAX - 64 && n_sealed >= 0 && n_sealed <= n_docs && post_len >= 0,
                 "tt_lexical_topk_postings: n_docs=%lld n_sealed=%lld post_len=%lld", (long long)n_docs, (long long)n_sealed,
                 (long long)post_len);
    TT_CHECK_ARG(out_scores && out_idx && thr_out && cnt_out && cand_cnt_out, "tt_lexical_topk_postings: null output");
    hipStream_t st = (hipStream_t)stream;
    if (n_docs == 0) {
        const int64_t n = (int64_t)n_q * k;
        hipLaunchKernelGGL(postings_pad_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, out_scores, out_idx, n, thr_out,
                           cnt_out, cand_cnt_out, n_q);
        TT_CHECK_LAUNCH();
        return TT_OK;
    }
    TT_CHECK_ARG(q_terms && q_weights && q_start && q_nnz && d_terms && d_weights && d_start && d_nnz,
                 "tt_lexical_topk_postings: null pointer");
    TT_CHECK_ARG(n_sealed == 0 || (range_lo && range_hi && range_start && (post_doc || post_len == 0)),
                 "tt_lexical_topk_postings: null posting arrays");
    const Layout l = layout_of(n_docs, n_sealed, n_q);
    if (!workspace || workspace_bytes < l.total) {
        tt_set_error("tt_lexical_topk_postings: workspace %zu < required %zu bytes", workspace_bytes, l.total);
        return TT_E_WORKSPACE;
    }
    char* ws = (char*)workspace;
    uint32_t* bitmap = (uint32_t*)ws;
    int32_t* blk = (int32_t*)(ws + l.off_blk);
    int32_t* cand = (int32_t*)(ws + l.off_cand);
    float* scores = (float*)(ws + l.off_scores);
    const int64_t tail = n_docs - n_sealed;
    {
        TtProfScope prof(TT_K_ROWOPS, st);
        if (l.nb > 0) {
            TT_CHECK_HIP(hipMemsetAsync(bitmap, 0, (size_t)n_q * l.words_q * sizeof(uint32_t), st));
            // grid_entries: the longest sum of range lengths of a query, as far as the caller knows it; the walk is grid-strided
            const int64_t mark_blocks = std::min<int64_t>(std::max<int64_t>((grid_entries + 255) / 256, 1), 2048);
            hipLaunchKernelGGL(postings_mark_kernel, dim3((unsigned)mark_blocks, (unsigned)n_q), dim3(256), 0, st, post_doc, post_len,
                               range_lo, range_hi, range_start, n_sealed, bitmap, l.words_q);
            TT_CHECK_LAUNCH();
            hipLaunchKernelGGL(postings_count_kernel, dim3((unsigned)l.nb, (unsigned)n_q), dim3(kSpanThreads), 0, st, bitmap, l.words_q,
                               l.nb, blk);
            TT_CHECK_LAUNCH();
        }
        hipLaunchKernelGGL((postings_scan_kernel<int32_t, int32_t>), dim3((unsigned)n_q), dim3(kScanThreads), 0, st, blk, (int64_t)l.nb,
                           (int64_t)(l.nb + 1), blk, (int64_t)(l.nb + 1), cand_cnt_out, (int32_t)tail);
        TT_CHECK_LAUNCH();
        if (l.nb > 0) {
            hipLaunchKernelGGL(postings_write_kernel, dim3((unsigned)l.nb, (unsigned)n_q), dim3(kSpanThreads), 0, st, bitmap, l.words_q,
                               l.nb, blk, cand, l.stride);
            TT_CHECK_LAUNCH();
        }
        if (tail > 0) {
            hipLaunchKernelGGL(postings_tail_kernel, dim3((unsigned)((tail + 255) / 256), (unsigned)n_q), dim3(256), 0, st, blk, l.nb,
                               n_sealed, n_docs, cand, l.stride);
            TT_CHECK_LAUNCH();
        }
    }
    // the scan's own scores: a tombstone's slot holds NaN, which the selection never returns
    const int64_t grid_cand = std::min<int64_t>(std::min<int64_t>(std::max<int64_t>(grid_entries, 0), n_sealed) + tail, n_docs);
    int rc = tt_lexical_score_lists(q_terms, q_weights, q_start, q_nnz, n_q, d_terms, d_weights, d_start, d_nnz, cand, cand_cnt_out,
                                    l.stride, (int)std::max<int64_t>(grid_cand, 1), __builtin_nanf(""), scores, st);
    if (rc) return rc;
    SelectParams se{};
    se.scores = scores;
    se.idx = cand;
    se.stride = l.stride;
    se.cnt = cand_cnt_out;
    se.m_fixed = 0;
    se.cap = (int)n_docs;
    se.idx_base = 0;
    se.k = k;
    se.out_scores = out_scores;
    se.out_idx = out_idx;
    se.out_stride = k;
    se.thr_out = thr_out;
    se.cnt_out = cnt_out;
    return tt_select_launch(se, n_q, st);
}

}  // extern "C"
