// Metadata filter -> ascending row list (tt_filter_rows, include/tt_hip.h), the first half of a filtered exact search.
//
// Every filterable metadata key is dictionary-encoded on the host (metadata_filter.py): one int32 code per row, 0 = key absent.
// Each clause of a filter is evaluated ONCE on the host over the key's distinct values and arrives here as a bitset over codes,
// so every operator (==, !=, <, in, contains, substring, ...) is the same device test:  bit[code[row]].  Up to
// TT_FILTER_MAX_CLAUSES clauses, combined with AND or OR.
//
// Three launches, no atomics, so the list comes out in ascending row order:
//   1. count : block b evaluates rows [lo + b T, lo + (b + 1) T), T = 4096; thread t owns rows lo + b T + 256 i + t (i < 16, coalesced
//              loads), keeps the 16 outcomes as a mask and the block writes its count
//   2. scan  : one block: exclusive scan of the block counts; the list offset of every segment boundary (matches below it) and the
//              total count
//   3. write : every block re-reads its masks and writes its matching rows at its scanned base, ordered (i, t) = ascending rows
// Traffic: 4 bytes per row per clause (codes) + 2 bytes per 16 rows (masks) + 4 bytes per listed row: HBM-bound, microseconds per
// million rows.  The list then drives tt_scan_topk_rows (scan_api.hip, the streaming scan through a gather).
#include <limits.h>

#include "common.h"

namespace {

constexpr int kFThreads = 256;
constexpr int kFRowsPerThread = 16;
constexpr int kFTile = kFThreads * kFRowsPerThread;   // rows per block
constexpr int kMaxClauses = 8;
constexpr int kMaxSegs = 64;

struct FilterParams {
    const int32_t* codes[kMaxClauses];     // [n_rows] per clause
    const uint32_t* bits[kMaxClauses];     // allowed-code bitsets, ceil(n_codes / 32) words
    int32_t n_codes[kMaxClauses];
    int n_clauses;
    int any;                               // 0 = AND, 1 = OR
    int64_t lo, hi;                        // rows [lo, hi) are evaluated
    int n_tiles;
    uint16_t* masks;                       // [n_tiles][256]
    int32_t* blk;                          // [n_tiles]: counts (pass 1), exclusive offsets (pass 2)
    int32_t* out_rows;
    int32_t* out_off;                      // [n_seg + 1]
    int n_seg;
    int64_t seg[kMaxSegs + 1];             // segment boundaries (rows), seg[0] = lo, seg[n_seg] = hi
};

__device__ __forceinline__ bool clause_ok(const FilterParams& p, int c, int64_t row) {
    const int32_t code = p.codes[c][row];
    // codes beyond the bitset: values the vocabulary learnt after the clause was compiled -- not allowed (code 0, key absent: bit 0 is never set)
    if ((uint32_t)code >= (uint32_t)p.n_codes[c]) return false;
    return (p.bits[c][code >> 5] >> (code & 31)) & 1u;
}

__global__ __launch_bounds__(kFThreads) void filter_count_kernel(FilterParams p) {
    __shared__ int wsum[kFThreads / TT_WAVE];
    const int tid = threadIdx.x;
    const int64_t base = p.lo + (int64_t)blockIdx.x * kFTile;
    uint32_t mask = 0;
#pragma unroll
    for (int i = 0; i < kFRowsPerThread; ++i) {
        const int64_t row = base + i * kFThreads + tid;
        if (row < p.hi) {
            bool ok = !p.any;
            for (int c = 0; c < p.n_clauses; ++c) {
                const bool m = clause_ok(p, c, row);
                ok = p.any ? (ok || m) : (ok && m);
            }
            mask |= (uint32_t)ok << i;
        }
    }
    p.masks[(size_t)blockIdx.x * kFThreads + tid] = (uint16_t)mask;
    int cnt = __popc(mask);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) cnt += __shfl_xor(cnt, o, 64);
    if ((tid & 63) == 0) wsum[tid >> 6] = cnt;
    __syncthreads();
    if (tid == 0) {
        int t = 0;
        for (int w = 0; w < kFThreads / TT_WAVE; ++w) t += wsum[w];
        p.blk[blockIdx.x] = t;
    }
}

// one block of 1024 threads: exclusive scan of the block counts in place, then the segment boundaries' list offsets
__global__ __launch_bounds__(1024) void filter_scan_kernel(FilterParams p) {
    __shared__ int wsum[16];
    __shared__ int carry;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    if (tid == 0) carry = 0;
    __syncthreads();
    for (int b0 = 0; b0 < p.n_tiles; b0 += 1024) {
        const int b = b0 + tid;
        const int v = b < p.n_tiles ? p.blk[b] : 0;
        int inc = v;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const int u = __shfl_up(inc, o, 64);
            if (lane >= o) inc += u;
        }
        if (lane == 63) wsum[wv] = inc;
        __syncthreads();
        int before = carry;
        for (int w = 0; w < wv; ++w) before += wsum[w];
        if (b < p.n_tiles) p.blk[b] = before + inc - v;
        __syncthreads();
        if (tid == 1023) carry = before + inc;
        __syncthreads();
    }
    const int total = carry;
    // boundary s: matches in rows [lo, seg[s]) = scanned base of its tile + the tile's matches below it (one wave per boundary)
    for (int s = wv; s <= p.n_seg; s += 16) {
        const int64_t rel = p.seg[s] - p.lo;
        const int64_t tile = rel / kFTile;
        int c = 0;
        if (s == p.n_seg || tile >= p.n_tiles) {
            c = total;
        } else {
            const int pos = (int)(rel - tile * kFTile);      // rows 256 i + t of the tile with 256 i + t < pos
            for (int t = lane; t < kFThreads; t += 64) {
                const int n_i = pos > t ? (pos - t + kFThreads - 1) / kFThreads : 0;
                const uint32_t m = p.masks[(size_t)tile * kFThreads + t] & ((1u << n_i) - 1u);
                c += __popc(m);
            }
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o, 64);
            c += p.blk[tile];
        }
        if (lane == 0) p.out_off[s] = c;
    }
}

__global__ __launch_bounds__(kFThreads) void filter_write_kernel(FilterParams p) {
    __shared__ int cnt[kFRowsPerThread][kFThreads / TT_WAVE];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const uint32_t mask = p.masks[(size_t)blockIdx.x * kFThreads + tid];
    const uint64_t below = (1ull << lane) - 1ull;
    int pre[kFRowsPerThread];
#pragma unroll
    for (int i = 0; i < kFRowsPerThread; ++i) {
        const uint64_t bal = __ballot((mask >> i) & 1u);
        pre[i] = __popcll(bal & below);
        if (lane == 0) cnt[i][wv] = __popcll(bal);
    }
    __syncthreads();
    int base = p.blk[blockIdx.x];
    const int64_t row0 = p.lo + (int64_t)blockIdx.x * kFTile;
#pragma unroll
    for (int i = 0; i < kFRowsPerThread; ++i) {
        int off = base;
        for (int w = 0; w < wv; ++w) off += cnt[i][w];
        if ((mask >> i) & 1u) p.out_rows[off + pre[i]] = (int32_t)(row0 + i * kFThreads + tid);
        for (int w = 0; w < kFThreads / TT_WAVE; ++w) base += cnt[i][w];
    }
}

size_t filter_layout(int64_t rows, size_t* off_blk) {
    const int64_t tiles = (rows + kFTile - 1) / kFTile;
    const size_t masks = tt_align_up((size_t)tiles * kFThreads * sizeof(uint16_t), 256);
    if (off_blk) *off_blk = masks;
    return masks + tt_align_up((size_t)(tiles > 0 ? tiles : 1) * sizeof(int32_t), 256);
}

}  // namespace

extern "C" {

size_t tt_filter_rows_workspace_bytes(int64_t n_rows) {
    if (n_rows < 0) return 0;
    return filter_layout(n_rows, nullptr);
}

int tt_filter_rows(int n_clauses, const int32_t* const* codes_host, const uint32_t* const* bitsets_host, const int32_t* n_codes_host,
                   int any, int64_t n_rows, const int64_t* seg_offsets_host, int n_segments, int32_t* out_rows, int32_t* out_offsets,
                   void* workspace, size_t workspace_bytes, void* stream) {
    TT_CHECK_ARG(n_clauses >= 1 && n_clauses <= kMaxClauses, "n_clauses=%d outside [1,%d]", n_clauses, kMaxClauses);
    TT_CHECK_ARG(codes_host && bitsets_host && n_codes_host, "null clause array");
    TT_CHECK_ARG(n_rows >= 0 && n_rows < (int64_t)INT32_MAX, "n_rows=%lld out of range", (long long)n_rows);
    TT_CHECK_ARG(n_segments >= 1 && n_segments <= kMaxSegs, "n_segments=%d outside [1,%d]", n_segments, kMaxSegs);
    TT_CHECK_ARG(out_rows && out_offsets, "null output pointer");
    FilterParams p{};
    p.n_clauses = n_clauses;
    p.any = any ? 1 : 0;
    for (int c = 0; c < n_clauses; ++c) {
        TT_CHECK_ARG(n_codes_host[c] >= 0, "clause %d: n_codes=%d", c, n_codes_host[c]);
        TT_CHECK_ARG(codes_host[c] && (bitsets_host[c] || n_codes_host[c] == 0), "clause %d: null code column or bitset", c);
        p.codes[c] = codes_host[c];
        p.bits[c] = bitsets_host[c];
        p.n_codes[c] = n_codes_host[c];
    }
    p.n_seg = n_segments;
    if (seg_offsets_host) {
        for (int s = 0; s <= n_segments; ++s) p.seg[s] = seg_offsets_host[s];
        TT_CHECK_ARG(p.seg[0] >= 0 && p.seg[n_segments] <= n_rows, "segment offsets outside [0, n_rows]");
        for (int s = 0; s < n_segments; ++s)
            TT_CHECK_ARG(p.seg[s] <= p.seg[s + 1], "segment offsets must be non-decreasing (segment %d)", s);
    } else {
        TT_CHECK_ARG(n_segments == 1, "n_segments=%d without segment offsets", n_segments);
        p.seg[0] = 0;
        p.seg[1] = n_rows;
    }
    p.lo = p.seg[0];
    p.hi = p.seg[n_segments];
    const int64_t rows = p.hi - p.lo;
    size_t off_blk = 0;
    const size_t need = filter_layout(rows, &off_blk);
    if (!workspace || workspace_bytes < need) {
        tt_set_error("tt_filter_rows: workspace %zu < required %zu bytes", workspace_bytes, need);
        return TT_E_WORKSPACE;
    }
    TT_CHECK_ARG(((uintptr_t)workspace % 256) == 0, "workspace must be 256-byte aligned");
    p.n_tiles = (int)((rows + kFTile - 1) / kFTile);
    p.masks = (uint16_t*)workspace;
    p.blk = (int32_t*)((char*)workspace + off_blk);
    p.out_rows = out_rows;
    p.out_off = out_offsets;
    hipStream_t st = (hipStream_t)stream;
    if (p.n_tiles > 0) {
        hipLaunchKernelGGL(filter_count_kernel, dim3(p.n_tiles), dim3(kFThreads), 0, st, p);
        TT_CHECK_LAUNCH();
    }
    hipLaunchKernelGGL(filter_scan_kernel, dim3(1), dim3(1024), 0, st, p);    // (no tiles: every offset is 0)
    TT_CHECK_LAUNCH();
    if (p.n_tiles > 0) {
        hipLaunchKernelGGL(filter_write_kernel, dim3(p.n_tiles), dim3(kFThreads), 0, st, p);
        TT_CHECK_LAUNCH();
    }
    return TT_OK;
}

}  // extern "C"
