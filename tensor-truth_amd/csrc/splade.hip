// SPLADE: learned sparse vectors from a masked-language-model head (include/tt_hip.h, "SPLADE").
//   tt_splade_pool[_f16]   out[b][v] = act(max over the rows r of sequence b of <t[r], E[v]> + bias[v]): the vocabulary projection and the
//                          maximum over a sequence's rows in one kernel -- the [rows][Vp] logits are never written
//   tt_sparse_compact      a dense fp32 weight row -> its positive entries as ascending (id, weight) pairs, at most max_terms of them
//
// The MFMA layout is multivec.hip's (mfma_f32_16x16x32: a lane's operand fragment is 16 contiguous bytes of one row, A rows / B columns
// on lane & 15, K offset 8 (lane >> 4); the accumulator of lane l holds rows 4 (l >> 4) + i, i = 0..3, of column l & 15).
//
// Compiled twice like the encoder path (common.h TT_F16): the bf16 object holds everything; the fp16 object tt_splade_pool_f16 alone.
#include "common.h"

#include <cmath>

namespace {

constexpr int kMaxH = 1024, kMaxVp = 65536, kMaxLen = 8192, kMaxSeq = 65535;
constexpr int kMaxTerms = 8192, kMaxV = 65536;

// ---- the vocabulary projection with a segmented maximum --------------------------------------------------------------------------
// One workgroup of four waves per (sequence, 256 vocabulary columns); workgroup numbers run over the sequences first, so that the
// workgroups in flight share one E tile (256 H elements: 384 KiB at H 768) through L2.  Wave w owns the 64 columns 64 w .. 64 w + 63 of
// the tile as four MFMA row blocks (A operand: 16 bytes of E's row); the sequence's rows are the MFMA's columns (B operand: 16 bytes
// of t's row), 64 of them -- four column blocks -- per pass.  A pass multiplies over all of K from a zero accumulator, k ascending in
// steps of 32 (the next step's fragments are loaded while the current step multiplies): the chain of a row's sum depends on H
// alone, and a row's place in a pass depends on its distance from the sequence's first row alone -- never on the start row, the
// batch or the grid.  Lane l then holds, for its column (a sequence row) and each of
// its 16 vocabulary rows, one finished dot product, and keeps the running maximum over the passes (rows past the sequence: -inf; their
// loads are clamped to the sequence's last row, so every load is in bounds).  The maximum is exact, associative and commutative: the
// 16 lanes of a vocabulary row meet in a butterfly at the end.  The bias is added and the activation applied once per column, after the
// maximum (fp32 rounding, relu and log1p are monotone: the same bits as applying them to every row first).  No LDS, no atomics, no
// initialisation pass: every element of out[b][0 .. Vp) is written exactly once.
constexpr int kPoolWaves = 4, kPoolVB = 4, kPoolRB = 4;
constexpr int kPoolTile = 16 * kPoolVB * kPoolWaves;      // vocabulary columns of a workgroup
constexpr int kPoolRows = 16 * kPoolRB;                   // sequence rows of a pass

__device__ __forceinline__ float max16(float v) {
    v = fmaxf(v, __shfl_xor(v, 1, 64));
    v = fmaxf(v, __shfl_xor(v, 2, 64));
    v = fmaxf(v, __shfl_xor(v, 4, 64));
    return fmaxf(v, __shfl_xor(v, 8, 64));
}

// the operand fragments of one k-step: 16 bytes of each of the lane's four t rows and four E rows
__device__ __forceinline__ void pool_load(uint4 (&tf)[kPoolRB], uint4 (&ef)[kPoolVB], const uint16_t* const (&trow)[kPoolRB],
                                          const uint16_t* erow, int H, int k0) {
#pragma unroll
    for (int rb = 0; rb < kPoolRB; ++rb) tf[rb] = *reinterpret_cast<const uint4*>(trow[rb] + k0);
#pragma unroll
    for (int vb = 0; vb < kPoolVB; ++vb) ef[vb] = *reinterpret_cast<const uint4*>(erow + (size_t)16 * vb * H + k0);
}

__device__ __forceinline__ void pool_mma(f32x4 (&acc)[kPoolVB][kPoolRB], const uint4 (&ef)[kPoolVB], const uint4 (&tf)[kPoolRB], int nrb) {
#pragma unroll
    for (int vb = 0; vb < kPoolVB; ++vb)
#pragma unroll
        for (int rb = 0; rb < kPoolRB; ++rb)
            if (rb < nrb) acc[vb][rb] = TT_MFMA_16x16x32(__builtin_bit_cast(ex8, ef[vb]), __builtin_bit_cast(ex8, tf[rb]), acc[vb][rb]);
}

__global__ __launch_bounds__(64 * kPoolWaves) void splade_pool_kernel(const uint16_t* __restrict__ t, int n_rows, int ld, int H,
                                                                      const uint16_t* __restrict__ E, const float* __restrict__ bias,
                                                                      int Vp, const int32_t* __restrict__ seq_start,
                                                                      const int32_t* __restrict__ seq_len, int n_seq, int max_len,
                                                                      int activation, float* __restrict__ out, int ldo) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, c = lane & 15, g = lane >> 4;
    const int b = blockIdx.x % n_seq;
    const int v0 = (blockIdx.x / n_seq) * kPoolTile + 16 * kPoolVB * wave;
    if (v0 >= Vp) return;   // (wave-uniform; Vp is a multiple of 128: the last tile may hold two live waves.  No barrier below.)
    const int s = seq_start[b];
    const int len = min(max(seq_len[b], 0), max_len);
    const int n = (s < 0 || s >= n_rows) ? 0 : min(len, n_rows - s);   // rows of the sequence inside [0, n_rows)
    float m[kPoolVB][4];
#pragma unroll
    for (int vb = 0; vb < kPoolVB; ++vb)
#pragma unroll
        for (int i = 0; i < 4; ++i) m[vb][i] = -INFINITY;
    const uint16_t* erow = E + (size_t)(v0 + c) * H + 8 * g;
    for (int r0 = 0; r0 < n; r0 += kPoolRows) {   // (workgroup-uniform)
        const int nrb = min(kPoolRB, (n - r0 + 15) >> 4);   // column blocks that hold a row of the sequence
        const uint16_t* trow[kPoolRB];
#pragma unroll
        for (int rb = 0; rb < kPoolRB; ++rb) trow[rb] = t + (size_t)(s + min(r0 + 16 * rb + c, n - 1)) * ld + 8 * g;
        f32x4 acc[kPoolVB][kPoolRB];
#pragma unroll
        for (int vb = 0; vb < kPoolVB; ++vb)
#pragma unroll
            for (int rb = 0; rb < kPoolRB; ++rb) acc[vb][rb] = f32x4{0.f, 0.f, 0.f, 0.f};
        // two register buffers: the fragments of step k + 32 are in flight while step k multiplies (H is a multiple of 64)
        uint4 tfa[kPoolRB], efa[kPoolVB], tfb[kPoolRB], efb[kPoolVB];
        pool_load(tfa, efa, trow, erow, H, 0);
        for (int k0 = 0; k0 < H; k0 += 64) {
            pool_load(tfb, efb, trow, erow, H, k0 + 32);
            pool_mma(acc, efa, tfa, nrb);
            if (k0 + 64 < H) pool_load(tfa, efa, trow, erow, H, k0 + 64);
            pool_mma(acc, efb, tfb, nrb);
        }
#pragma unroll
        for (int rb = 0; rb < kPoolRB; ++rb) {
            const bool live = rb < nrb && r0 + 16 * rb + c < n;
#pragma unroll
            for (int vb = 0; vb < kPoolVB; ++vb)
#pragma unroll
                for (int i = 0; i < 4; ++i) m[vb][i] = fmaxf(m[vb][i], live ? acc[vb][rb][i] : -INFINITY);
        }
    }
    float* orow = out + (size_t)b * ldo;
#pragma unroll
    for (int vb = 0; vb < kPoolVB; ++vb) {
        const float m0 = max16(m[vb][0]), m1 = max16(m[vb][1]), m2 = max16(m[vb][2]), m3 = max16(m[vb][3]);
        if (c < 4) {   // lane c of a group writes vocabulary row 4 g + c of the block
            const int v = v0 + 16 * vb + 4 * g + c;
            const float x = (c == 0 ? m0 : c == 1 ? m1 : c == 2 ? m2 : m3) + bias[v];
            orow[v] = activation ? log1pf(fmaxf(x, 0.f)) : x;
        }
    }
}

#if !TT_F16
// ---- a dense weight row -> ascending (id, weight) pairs ---------------------------------------------------------------------------
// One workgroup of 1024 threads per row.  An entry qualifies when its BITS are those of a positive number or +inf (0 < bits <=
// 0x7f800000: an integer test, so a denormal qualifies whatever the float mode; a NaN, a zero of either sign and a negative do not);
// for such entries the order of the bits is the order of the values.  A radix select over the bits, one byte per pass from the top (a
// 256-bin histogram in LDS: integer counts, whose order of arrival does not show), finds the max_terms-th largest value T and how
// many of the entries equal to T are kept (`need`: the lowest ids); with at most max_terms qualifying entries the first pass ends
// the select and everything is kept.  The last pass walks the ids in ascending order, 1024 at a time, with two workgroup-wide prefix
// counts (entries equal to T so far; entries kept so far): an entry's slot is the number of kept entries below it.
constexpr int kCompactThreads = 1024, kCompactWaves = kCompactThreads / 64;

__device__ __forceinline__ uint32_t weight_key(const float* row, int i) {
    const uint32_t u = __float_as_uint(row[i]);
    return u - 1u < 0x7f800000u ? u : 0u;
}

__global__ __launch_bounds__(kCompactThreads) void sparse_compact_kernel(const float* __restrict__ w, int ldw, int V, int max_terms,
                                                                         int32_t* __restrict__ out_terms, float* __restrict__ out_weights,
                                                                         int32_t* __restrict__ out_nnz) {
    __shared__ uint32_t hist[256];
    __shared__ uint32_t sel[3];                          // prefix, remaining rank, done
    __shared__ int cnt_eq[kCompactWaves], cnt_keep[kCompactWaves];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const float* row = w + (size_t)blockIdx.x * ldw;
    int32_t* terms = out_terms + (size_t)blockIdx.x * max_terms;
    float* weights = out_weights + (size_t)blockIdx.x * max_terms;
    uint32_t prefix = 0, mask = 0, rank = (uint32_t)max_terms, done = 0;
    for (int pass = 0; pass < 4 && !done; ++pass) {   // (workgroup-uniform)
        const int shift = 24 - 8 * pass;
        if (tid < 256) hist[tid] = 0;
        __syncthreads();
        for (int i = tid; i < V; i += kCompactThreads) {
            const uint32_t key = weight_key(row, i);
            if (key != 0 && (key & mask) == prefix) atomicAdd(&hist[(key >> shift) & 255u], 1u);
        }
        __syncthreads();
        if (tid == 0) {
            uint32_t above = 0;
            int d = 255;
            for (; d > 0 && above + hist[d] < rank; --d) above += hist[d];
            // pass 0 counts every qualifying entry: with no more than max_terms of them there is no cut
            if (above + hist[d] < rank) {
                sel[0] = 0; sel[1] = 0; sel[2] = 1;
            } else {
                sel[0] = prefix | ((uint32_t)d << shift); sel[1] = rank - above; sel[2] = 0;
            }
        }
        __syncthreads();
        prefix = sel[0]; rank = sel[1]; done = sel[2];
        mask |= 255u << shift;
    }
    // (a select that ran out before its fourth pass had fewer entries left than the rank at some level, which the first pass alone can)
    const uint32_t T = done ? 0u : prefix;
    const int need = done ? 0 : (int)rank;
    int base_eq = 0, base_keep = 0;
    for (int i0 = 0; i0 < V; i0 += kCompactThreads) {   // (workgroup-uniform)
        const int i = i0 + tid;
        const uint32_t key = i < V ? weight_key(row, i) : 0u;
        const bool eq = T != 0 && key == T;
        const unsigned long long below = (1ull << lane) - 1ull;
        const unsigned long long beq = __ballot(eq);
        if (lane == 0) cnt_eq[wave] = __popcll(beq);
        __syncthreads();
        int eq_rank = base_eq + __popcll(beq & below), eq_all = 0;
#pragma unroll
        for (int x = 0; x < kCompactWaves; ++x) {
            const int n = cnt_eq[x];
            eq_rank += x < wave ? n : 0;
            eq_all += n;
        }
        const bool keep = key > T || (eq && eq_rank < need);
        const unsigned long long bkeep = __ballot(keep);
        if (lane == 0) cnt_keep[wave] = __popcll(bkeep);
        __syncthreads();
        int slot = base_keep + __popcll(bkeep & below), keep_all = 0;
#pragma unroll
        for (int x = 0; x < kCompactWaves; ++x) {
            const int n = cnt_keep[x];
            slot += x < wave ? n : 0;
            keep_all += n;
        }
        if (keep && slot < max_terms) {
            terms[slot] = i;
            weights[slot] = __uint_as_float(key);
        }
        base_eq += eq_all;
        base_keep += keep_all;
        __syncthreads();   // the counts are read before the next round writes them
    }
    const int nnz = min(base_keep, max_terms);
    if (tid == 0) out_nnz[blockIdx.x] = nnz;
    for (int j = nnz + tid; j < max_terms; j += kCompactThreads) {
        terms[j] = -1;
        weights[j] = 0.f;
    }
}
#endif

}  // namespace

extern "C" {

int tt_splade_pool(const void* t, int n_rows, int ld, int H, const void* E, const float* bias, int Vp, const int32_t* seq_start,
                   const int32_t* seq_len, int n_seq, int max_len, int activation, float* out, int ldo, void* stream) {
    const char* name = kF16 ? "tt_splade_pool_f16" : "tt_splade_pool";
    if (H <= 0 || H % 128 || H > kMaxH) {
        tt_set_error("%s: hidden=%d must be a multiple of 128 and <= %d", name, H, kMaxH);
        return TT_E_UNSUPPORTED;
    }
    if (Vp <= 0 || Vp % 128 || Vp > kMaxVp) {
        tt_set_error("%s: Vp=%d must be a multiple of 128 and <= %d", name, Vp, kMaxVp);
        return TT_E_UNSUPPORTED;
    }
    if (max_len < 1 || max_len > kMaxLen) {
        tt_set_error("%s: max_len=%d must be 1 .. %d", name, max_len, kMaxLen);
        return TT_E_UNSUPPORTED;
    }
    if (n_seq < 0 || n_seq > kMaxSeq) {
        tt_set_error("%s: n_seq=%d must be 0 .. %d", name, n_seq, kMaxSeq);
        return TT_E_UNSUPPORTED;
    }
    TT_CHECK_ARG(n_rows >= 0 && ld >= H && ld % 8 == 0 && ldo >= Vp && (activation == 0 || activation == 1),
                 "%s: n_rows=%d ld=%d (>= hidden=%d, a multiple of 8) ldo=%d (>= Vp=%d) activation=%d (0 or 1)", name, n_rows, ld, H, ldo,
                 Vp, activation);
    if (n_seq == 0) return TT_OK;
    TT_CHECK_ARG(t && E && bias && seq_start && seq_len && out, "%s: null pointer", name);
    hipStream_t st = (hipStream_t)stream;
    const unsigned tiles = (unsigned)((Vp + kPoolTile - 1) / kPoolTile);
    TtProfScope prof(TT_K_GEMM, st);
    hipLaunchKernelGGL(splade_pool_kernel, dim3(tiles * (unsigned)n_seq), dim3(64 * kPoolWaves), 0, st, (const uint16_t*)t, n_rows, ld, H,
                       (const uint16_t*)E, bias, Vp, seq_start, seq_len, n_seq, max_len, activation, out, ldo);
    TT_CHECK_LAUNCH();
    return TT_OK;
}

#if !TT_F16
int tt_sparse_compact(const float* w, int ldw, int V, int n_seq, int max_terms, int32_t* out_terms, float* out_weights, int32_t* out_nnz,
                      void* stream) {
    if (V < 1 || V > kMaxV) {
        tt_set_error("tt_sparse_compact: V=%d must be 1 .. %d", V, kMaxV);
        return TT_E_UNSUPPORTED;
    }
    if (max_terms < 1 || max_terms > kMaxTerms) {
        tt_set_error("tt_sparse_compact: max_terms=%d must be 1 .. %d", max_terms, kMaxTerms);
        return TT_E_UNSUPPORTED;
    }
    TT_CHECK_ARG(n_seq >= 0 && ldw >= V, "tt_sparse_compact: n_seq=%d ldw=%d V=%d", n_seq, ldw, V);
    if (n_seq == 0) return TT_OK;
    TT_CHECK_ARG(w && out_terms && out_weights && out_nnz, "tt_sparse_compact: null pointer");
    hipStream_t st = (hipStream_t)stream;
    TtProfScope prof(TT_K_ROWOPS, st);
    hipLaunchKernelGGL(sparse_compact_kernel, dim3((unsigned)n_seq), dim3(kCompactThreads), 0, st, w, ldw, V, max_terms, out_terms,
                       out_weights, out_nnz);
    TT_CHECK_LAUNCH();
    return TT_OK;
}
#endif

}  // extern "C"
