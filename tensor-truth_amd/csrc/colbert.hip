// Late-interaction (ColBERT) reranking and retrieval: the kernels only this family needs (include/tt_hip.h, "ColBERT late interaction").
//   tt_maxsim              scores[q][c] = sum_i max_j <Q_i, D_j> over token vectors that already sit in device memory
//   tt_maxsim_scan_topk    that score for every stored document in one read of the store, then the library's exact selection (select.hip)
//   tt_colbert_project     v = normalize(W h) for the listed rows of a hidden state, one rounding to the element type
//   tt_attention_keylimit  attention in which every row of a sequence is a query and only its first key_len rows are keys
//                          (a ColBERT query: [MASK] expansion tokens are encoded and scored, never attended to)
// The encoder itself is encoder_api.hip's (tt_encoder_forward_keylen: the BERT forward with the third kernel in every layer).
//
// All but the scan (which stages its queries in LDS) are one-wave MFMA tiles without LDS staging: a lane's operand fragment of
// mfma_f32_16x16x32 is 16 contiguous bytes of one row.  The layout is attention_tile's (varlen.h): A rows on lane & 15, K offset 8 (lane >> 4); the accumulator of lane l holds rows
// 4 (l >> 4) + i, i = 0..3, of column l & 15.
//
// Compiled twice like the encoder path (common.h TT_F16): bf16 and fp16 (external names with an _f16 suffix, f16_names.h).
#include "common.h"
#include "encoder.h"
#include "scan.h"

#include <limits.h>

#include <algorithm>

namespace {

// maximum over the four lanes l, l ^ 16, l ^ 32, l ^ 48: one column of an MFMA 16x16 result (varlen.h's wave_max16)
__device__ __forceinline__ float wave_max16(float v) {
    v = fmaxf(v, __shfl_xor(v, 16, 64));
    return fmaxf(v, __shfl_xor(v, 32, 64));
}

constexpr int kMaxsimWaves = 2;      // query blocks of 16 tokens a workgroup works on at a time (a 32-token query: one pass)
constexpr int kMaxQueryLen = 128, kMaxDocLen = 512, kMaxDim = 128;

// ---- MaxSim ---------------------------------------------------------------------------------------------------------------------
// One workgroup per (candidate, query).  Wave w takes the query blocks w, w + kMaxsimWaves, ...: the block's 16 query tokens are the
// MFMA's columns (B operand, dim / 32 fragments held in registers), the document's tokens its rows, 16 per step.  Lane l keeps the
// running maximum of its four document rows of query column l & 15 (rows past d_len: -inf); one exchange across the four lane groups
// finishes the maximum, which goes to LDS.  Thread 0 then adds the q_len maxima in index order in fp32: a score depends on its own
// pair alone.  Lengths beyond the limits the entry point documents are clamped, so a bad length array cannot read past a buffer the
// host sized by those limits.
template <int DIM>
__global__ __launch_bounds__(64 * kMaxsimWaves) void maxsim_kernel(const uint16_t* __restrict__ qv, const int32_t* __restrict__ q_start,
                                                                   const int32_t* __restrict__ q_len, const uint16_t* __restrict__ dv,
                                                                   const int64_t* __restrict__ d_start,
                                                                   const int32_t* __restrict__ d_len, const int32_t* __restrict__ cand,
                                                                   int n_cand, float* __restrict__ scores) {
    __shared__ float tok_max[kMaxQueryLen];
    const int ci = blockIdx.x, q = blockIdx.y;
    const int doc = cand ? cand[(size_t)q * n_cand + ci] : ci;
    float* dst = scores + (size_t)q * n_cand + ci;
    if (doc < 0) {   // (workgroup-uniform)
        if (threadIdx.x == 0) *dst = -INFINITY;
        return;
    }
    const int ql = min(max(q_len[q], 0), kMaxQueryLen), dl = min(max(d_len[doc], 0), kMaxDocLen);
    if (dl == 0 || ql == 0) {
        if (threadIdx.x == 0) *dst = 0.f;
        return;
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, c = lane & 15, g = lane >> 4;
    const uint16_t* qbase = qv + (size_t)q_start[q] * DIM + 8 * g;
    const uint16_t* dbase = dv + (size_t)d_start[doc] * DIM + 8 * g;
    const uint4 zero4 = uint4{0u, 0u, 0u, 0u};
    for (int q0 = 16 * wave; q0 < ql; q0 += 16 * kMaxsimWaves) {   // (wave-uniform)
        ex8 qf[DIM / 32];
#pragma unroll
        for (int kk = 0; kk < DIM / 32; ++kk) {
            const uint4 u = q0 + c < ql ? *reinterpret_cast<const uint4*>(qbase + (size_t)(q0 + c) * DIM + kk * 32) : zero4;
            qf[kk] = __builtin_bit_cast(ex8, u);
        }
        float m = -INFINITY;
        for (int d0 = 0; d0 < dl; d0 += 16) {
            f32x4 s = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int kk = 0; kk < DIM / 32; ++kk) {
                const uint4 u = d0 + c < dl ? *reinterpret_cast<const uint4*>(dbase + (size_t)(d0 + c) * DIM + kk * 32) : zero4;
                s = TT_MFMA_16x16x32(__builtin_bit_cast(ex8, u), qf[kk], s);
            }
#pragma unroll
            for (int i = 0; i < 4; ++i) m = fmaxf(m, d0 + 4 * g + i < dl ? s[i] : -INFINITY);
        }
        m = wave_max16(m);
        if (g == 0 && q0 + c < ql) tok_max[q0 + c] = m;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        float acc = 0.f;
        for (int i = 0; i < ql; ++i) acc += tok_max[i];
        *dst = acc;
    }
}

// ---- MaxSim over the whole store ----------------------------------------------------------------------------------------------
// tt_maxsim_scan_topk's scoring pass: every document is read ONCE and scored against every query of the pass.  A persistent grid of
// four-wave workgroups; a wave owns whole documents, taken in a static grid-stride walk over chunks of kScanChunk consecutive document
// numbers -- no atomics, nothing crosses a wave.
//   Queries: the B fragments of up to kScanBlocks 16-token query blocks (256 padded query rows: 64 KB at dim 128, the LDS budget of a
//     pass) are staged once per workgroup in fragment order -- qfrag[(block * DIM/32 + kk) * 64 + lane] is the 16 bytes lane `lane`
//     feeds the MFMA, so a wave's ds_read_b128 covers 1 KB of consecutive addresses (conflict-free).  Rows past q_len are zeros, as in
//     maxsim_kernel.  Queries that do not fit are taken by further passes INSIDE the launch (the lengths live on the device; every
//     workgroup plans the same split): each pass is one sweep of the store into its own workspace rows.
//   Documents: a 16-token tile is loaded once into registers as A fragments (16 contiguous bytes of one row per lane and kk, as in
//     maxsim_kernel) and reused against every block of the pass; the NEXT tile of the wave's walk -- of this document or of the next
//     live one -- is loaded into a second register buffer before the current tile's MFMAs are issued.
//   Per (query block, lane) one running maximum in a register.  At a document's last tile the maxima are finished across the four lane
//     groups (wave_max16), go to the wave's own LDS strip, and lane j adds the q_len maxima of the pass's query j in index order in
//     fp32.  The chain per <Q_i, D_j>, the masking, the order of the fmaxf calls per lane and the sum are maxsim_kernel's: the same bits.
//   A dead document (alive[doc] == 0) writes NaN without being read; a live one of length 0 writes 0.
constexpr int kScanWaves = 4;       // waves per workgroup
constexpr int kScanChunk = 2;       // consecutive documents a wave takes per step of its walk
constexpr int kScanBlocks = 16;     // 16-token query blocks per pass
constexpr int kScanWgPerCu = 2;     // workgroups the grid holds per compute unit: 2 x (64 KB of fragments + 6 KB) of its 160 KB
constexpr int kScanMaxQueries = 64;

template <int DIM>
__global__ __launch_bounds__(64 * kScanWaves) void maxsim_scan_kernel(const uint16_t* __restrict__ qv, const int32_t* __restrict__ q_start,
                                                                      const int32_t* __restrict__ q_len, int n_q,
                                                                      const uint16_t* __restrict__ dv, const int64_t* __restrict__ d_start,
                                                                      const int32_t* __restrict__ d_len, const uint8_t* __restrict__ alive,
                                                                      int n_docs, float* __restrict__ ws, int64_t stride) {
    constexpr int KK = DIM / 32;
    __shared__ uint4 qfrag[kScanBlocks * KK * 64];
    __shared__ float tok_max[kScanWaves][16 * kScanBlocks + kScanMaxQueries];   // (query j's maxima start j words late: no bank is shared)
    __shared__ int q_first[kScanMaxQueries], q_rows[kScanMaxQueries];           // per query of the pass: its first block, its length
    __shared__ int blk_q[kScanBlocks], blk_row[kScanBlocks];                    // per block: its query within the pass, its first row
    __shared__ int pass_end, pass_blocks;
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), c = lane & 15, g = lane >> 4;
    const int64_t n_waves = (int64_t)gridDim.x * kScanWaves;
    const uint4 zero4 = uint4{0u, 0u, 0u, 0u};
    float* tm = tok_max[wave];

    for (int q_lo = 0; q_lo < n_q;) {   // (workgroup-uniform: one pass per turn)
        if (threadIdx.x == 0) {
            int nb = 0, q = q_lo;
            for (; q < n_q; ++q) {
                const int ql = min(max(q_len[q], 0), kMaxQueryLen), b = (ql + 15) >> 4;
                if (nb + b > kScanBlocks) break;   // (a query holds at most 8 blocks: every pass takes at least one)
                q_first[q - q_lo] = nb;
                q_rows[q - q_lo] = ql;
                for (int i = 0; i < b; ++i) {
                    blk_q[nb + i] = q - q_lo;
                    blk_row[nb + i] = 16 * i;
                }
                nb += b;
            }
            pass_end = q;
            pass_blocks = nb;
        }
        __syncthreads();
        const int q_hi = __builtin_amdgcn_readfirstlane(pass_end), nb = __builtin_amdgcn_readfirstlane(pass_blocks), nq = q_hi - q_lo;
        for (int idx = threadIdx.x; idx < nb * KK * 64; idx += 64 * kScanWaves) {
            const int l = idx & 63, kk = (idx >> 6) % KK, b = (idx >> 6) / KK;
            const int qi = blk_q[b], row = blk_row[b] + (l & 15);
            uint4 u = zero4;
            if (row < q_rows[qi])
                u = *reinterpret_cast<const uint4*>(qv + ((size_t)q_start[q_lo + qi] + row) * DIM + kk * 32 + 8 * (l >> 4));
            qfrag[idx] = u;
        }
        __syncthreads();

        // the wave's walk, one tile ahead: (doc, d0) is the tile that is loaded next
        int64_t chunk = (int64_t)blockIdx.x * kScanWaves + wave - n_waves;
        int in_chunk = kScanChunk - 1, doc = -1, dl = 0, d0 = 0;
        bool more = true;
        const uint16_t* base = dv;
        auto advance = [&]() {
            d0 += 16;
            while (d0 >= dl) {
                if (++in_chunk == kScanChunk) {
                    in_chunk = 0;
                    chunk += n_waves;
                }
                const int64_t d = chunk * kScanChunk + in_chunk;
                if (d >= n_docs) {
                    more = false;
                    return;
                }
                doc = (int)d;
                const bool live = !alive || alive[doc] != 0;
                dl = live ? min(max(d_len[doc], 0), kMaxDocLen) : 0;
                d0 = 0;
                if (dl == 0) {
                    if (lane < nq) ws[(size_t)(q_lo + lane) * stride + doc] = live ? 0.f : __builtin_nanf("");
                } else {
                    base = dv + (size_t)d_start[doc] * DIM + 8 * g;
                }
            }
        };
        auto load = [&](uint4(&a)[KK]) {
#pragma unroll
            for (int kk = 0; kk < KK; ++kk)
                a[kk] = d0 + c < dl ? *reinterpret_cast<const uint4*>(base + (size_t)(d0 + c) * DIM + kk * 32) : zero4;
        };

        float m[kScanBlocks];
#pragma unroll
        for (int b = 0; b < kScanBlocks; ++b) m[b] = -INFINITY;
        uint4 a0[KK], a1[KK];
        advance();
        bool have = more;
        if (have) load(a0);
        while (have) {   // (wave-uniform)
            const int cdoc = doc, cdl = dl, cd0 = d0;
            advance();
            if (more) load(a1);
#pragma unroll
            for (int b = 0; b < kScanBlocks; ++b) {
                if (b < nb) {
                    f32x4 s = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
                    for (int kk = 0; kk < KK; ++kk)
                        s = TT_MFMA_16x16x32(__builtin_bit_cast(ex8, a0[kk]), __builtin_bit_cast(ex8, qfrag[(b * KK + kk) * 64 + lane]), s);
#pragma unroll
                    for (int i = 0; i < 4; ++i) m[b] = fmaxf(m[b], cd0 + 4 * g + i < cdl ? s[i] : -INFINITY);
                }
            }
            if (cd0 + 16 >= cdl) {   // the document's last tile: finish its maxima and add them up
#pragma unroll
                for (int b = 0; b < kScanBlocks; ++b) {
                    if (b < nb) {
                        const float v = wave_max16(m[b]);
                        if (g == 0) tm[16 * b + c + blk_q[b]] = v;
                        m[b] = -INFINITY;
                    }
                }
                asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
                __builtin_amdgcn_wave_barrier();
                if (lane < nq) {
                    const float* t = tm + 16 * q_first[lane] + lane;
                    const int n = q_rows[lane];
                    float acc = 0.f;
                    for (int i = 0; i < n; ++i) acc += t[i];
                    ws[(size_t)(q_lo + lane) * stride + cdoc] = acc;
                }
                asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
                __builtin_amdgcn_wave_barrier();
            }
#pragma unroll
            for (int kk = 0; kk < KK; ++kk) a0[kk] = a1[kk];
            have = more;
        }
        __syncthreads();   // (the next pass restages the fragments and the tables)
        q_lo = q_hi;
    }
}

__global__ void maxsim_scan_pad_kernel(float* __restrict__ out_scores, int32_t* __restrict__ out_idx, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) {
        out_scores[i] = -INFINITY;
        out_idx[i] = -1;
    }
}

// ---- projection + L2 normalisation of listed rows ----------------------------------------------------------------------------
// One workgroup of four waves per 16 output rows.  The output rows are the MFMA's columns (B operand: 16 bytes of the source row
// rows[n]), W's rows its rows; wave w owns the 16-wide slices w, w + 4 of dim.  The squared norm of a row is summed per lane over
// its values, across the four lane groups, then across the waves through LDS in wave order: a row's bits do not depend on where in
// a launch it sits.  A source row outside [0, n_rows) projects a zero row.
constexpr int kProjWaves = 4;

__global__ __launch_bounds__(64 * kProjWaves) void colbert_project_kernel(const uint16_t* __restrict__ hidden, int n_rows, int H,
                                                                          const uint16_t* __restrict__ W, int dim,
                                                                          const int32_t* __restrict__ rows, int n_out,
                                                                          uint16_t* __restrict__ out) {
    __shared__ float part[kProjWaves][16];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, c = lane & 15, g = lane >> 4;
    const int n = blockIdx.x * 16 + c;
    const int src = n < n_out ? rows[n] : -1;
    const bool live = src >= 0 && src < n_rows;
    const uint16_t* hrow = hidden + (size_t)(live ? src : 0) * H + 8 * g;
    const uint4 zero4 = uint4{0u, 0u, 0u, 0u};
    constexpr int kTiles = kMaxDim / 16 / kProjWaves;   // 16-wide slices of dim per wave
    f32x4 acc[kTiles];
#pragma unroll
    for (int t = 0; t < kTiles; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int k0 = 0; k0 < H; k0 += 32) {
        const ex8 hf = __builtin_bit_cast(ex8, live ? *reinterpret_cast<const uint4*>(hrow + k0) : zero4);
#pragma unroll
        for (int t = 0; t < kTiles; ++t) {
            const int r = 16 * (wave + kProjWaves * t) + c;   // W row of this lane's A fragment
            const uint4 u = r < dim ? *reinterpret_cast<const uint4*>(W + (size_t)r * H + k0 + 8 * g) : zero4;
            acc[t] = TT_MFMA_16x16x32(__builtin_bit_cast(ex8, u), hf, acc[t]);
        }
    }
    float ss = 0.f;   // (slices past dim hold zeros)
#pragma unroll
    for (int t = 0; t < kTiles; ++t)
#pragma unroll
        for (int i = 0; i < 4; ++i) ss += acc[t][i] * acc[t][i];
    ss += __shfl_xor(ss, 16, 64);
    ss += __shfl_xor(ss, 32, 64);
    if (g == 0) part[wave][c] = ss;
    __syncthreads();
    float tot = part[0][c];
#pragma unroll
    for (int w = 1; w < kProjWaves; ++w) tot += part[w][c];
    const float den = fmaxf(sqrtf(tot), 1e-12f);
    if (n < n_out) {
#pragma unroll
        for (int t = 0; t < kTiles; ++t) {
            const int col = 16 * (wave + kProjWaves * t) + 4 * g;
            if (col < dim)
                *reinterpret_cast<uint2*>(out + (size_t)n * dim + col) =
                    uint2{pack_e2(acc[t][0] / den, acc[t][1] / den), pack_e2(acc[t][2] / den, acc[t][3] / den)};
        }
    }
}

// ---- key-limited attention over packed varlen sequences ------------------------------------------------------------------------
// attention_tile's arithmetic (varlen.h: S^T = K Q^T with permuted K rows, fp32 softmax in the log2 domain with a running maximum,
// P rounded to the element type, O^T += V^T P^T from the V8 layout) for sequences of up to 128 rows, at any start row: one wave per
// (16-query tile, sequence, head); the queries are all seq_len rows, the keys the rows s0 .. s0 + key_len - 1.  Key blocks are
// walked on the batch's 8-row grid from the group that holds s0, as the tile does; a neighbour's rows in a shared group are
// masked.  No row at or behind s0 + key_len is read as a key, and no V group that holds none of them.  key_len is clamped into
// [1, seq_len]: the first block holds row s0, a live key for every query.
template <int D>
__global__ __launch_bounds__(64) void keylimit_attention_kernel(const uint16_t* __restrict__ qk, int ld, int q_col0, int k_col0,
                                                                const uint16_t* __restrict__ vt, int ldvt, uint16_t* __restrict__ out,
                                                                int ld_out, const int32_t* __restrict__ seq_start,
                                                                const int32_t* __restrict__ seq_len,
                                                                const int32_t* __restrict__ key_len, int n_seq, float scale_log2) {
    const int t = blockIdx.x, h = blockIdx.z;
    const int lane = threadIdx.x, c = lane & 15, g = lane >> 4;
    const uint4 zero4 = uint4{0u, 0u, 0u, 0u};
    for (int b = blockIdx.y; b < n_seq; b += gridDim.y) {   // (wave-uniform: every lane takes the same sequences)
        const int s0 = seq_start[b], L = min(seq_len[b], kMaxQueryLen);
        if (s0 < 0 || 16 * t >= L) continue;
        const int s_end = s0 + L, k_end = s0 + min(max(key_len[b], 1), L);
        const int qrow = s0 + 16 * t + c;
        ex8 qf[D / 32];
#pragma unroll
        for (int kk = 0; kk < D / 32; ++kk) {
            const uint4 u = qrow < s_end ? *reinterpret_cast<const uint4*>(qk + (size_t)qrow * ld + q_col0 + h * D + kk * 32 + 8 * g)
                                         : zero4;
            qf[kk] = __builtin_bit_cast(ex8, u);
        }
        f32x4 o[D / 16];
#pragma unroll
        for (int dt = 0; dt < D / 16; ++dt) o[dt] = f32x4{0.f, 0.f, 0.f, 0.f};
        float m = -1e30f, l = 0.f;
        const uint16_t* kbase = qk + k_col0 + (size_t)h * D + 8 * g;
        const uint16_t* vbase = vt + ((size_t)h * D + c) * 8;
        for (int kb = s0 & ~7; kb < k_end; kb += 32) {
            f32x4 s[2];
#pragma unroll
            for (int tt = 0; tt < 2; ++tt) {
                // A row c of tile tt is key kb + 8 (c >> 2) + 4 tt + (c & 3): result row 4 g + i is then key kb + 8 g + 4 tt + i
                const int krow = kb + 8 * (c >> 2) + 4 * tt + (c & 3);
                s[tt] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int kk = 0; kk < D / 32; ++kk) {
                    const uint4 u = krow < k_end ? *reinterpret_cast<const uint4*>(kbase + (size_t)krow * ld + kk * 32) : zero4;
                    s[tt] = TT_MFMA_16x16x32(__builtin_bit_cast(ex8, u), qf[kk], s[tt]);
                }
            }
            float x[8];
            float bm = -INFINITY;
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const int key = kb + 8 * g + j;
                x[j] = (key >= s0 && key < k_end) ? s[j >> 2][j & 3] * scale_log2 : -INFINITY;
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
            const int grp = (kb >> 3) + g;      // V^T fragment: feature 16 dt + c, keys kb + 8 g .. + 7
            const bool vok = 8 * grp < k_end;
#pragma unroll
            for (int dt = 0; dt < D / 16; ++dt) {
                const uint4 u = vok ? *reinterpret_cast<const uint4*>(vbase + (size_t)grp * ldvt + (size_t)dt * 16 * 8) : zero4;
                o[dt] = TT_MFMA_16x16x32(__builtin_bit_cast(ex8, u), pf, o[dt] * alpha);
            }
        }
        l += __shfl_xor(l, 16, 64);
        l += __shfl_xor(l, 32, 64);
        if (qrow < s_end) {   // (the only lane-dependent branch: the wave is whole again for the next sequence)
            const float inv = 1.0f / l;
            uint16_t* dst = out + (size_t)qrow * ld_out + h * D + 4 * g;
#pragma unroll
            for (int dt = 0; dt < D / 16; ++dt)
                *reinterpret_cast<uint2*>(dst + dt * 16) = uint2{pack_e2(o[dt][0] * inv, o[dt][1] * inv),
                                                                 pack_e2(o[dt][2] * inv, o[dt][3] * inv)};
        }
    }
}

template <int DIM>
void maxsim_launch(const uint16_t* q, const int32_t* q_start, const int32_t* q_len, int n_q, const uint16_t* d, const int64_t* d_start,
                   const int32_t* d_len, const int32_t* cand, int n_cand, float* scores, hipStream_t st) {
    hipLaunchKernelGGL(maxsim_kernel<DIM>, dim3(n_cand, n_q), dim3(64 * kMaxsimWaves), 0, st, q, q_start, q_len, d, d_start, d_len,
                       cand, n_cand, scores);
}

}  // namespace

int tt_attention_keylimit_launch(const AttnParams& p, const int32_t* key_len, hipStream_t st) {
    TT_CHECK_ARG(key_len != nullptr, "null key_len");
    if (p.head_dim != 64 && p.head_dim != 32) {
        tt_set_error("key-limited attention: head_dim=%d (supported: 32, 64)", p.head_dim);
        return TT_E_UNSUPPORTED;
    }
    if (p.max_len <= 0 || p.max_len > kMaxQueryLen) {
        tt_set_error("key-limited attention: max_len=%d (sequences of 1 .. %d rows)", p.max_len, kMaxQueryLen);
        return TT_E_UNSUPPORTED;
    }
    TT_CHECK_ARG(p.heads > 0 && p.n_seq > 0, "heads=%d n_seq=%d", p.heads, p.n_seq);
    TT_CHECK_ARG(p.ld_qk % 8 == 0 && p.q_col0 % 8 == 0 && p.k_col0 % 8 == 0 && p.q_col0 >= 0 && p.k_col0 >= 0 && p.ld_out % 4 == 0 &&
                     p.ld_qk >= std::max(p.q_col0, p.k_col0) + p.heads * p.head_dim && p.ld_out >= p.heads * p.head_dim &&
                     p.ldvt >= 8 * p.heads * p.head_dim && p.ldvt % 8 == 0,
                 "ld_qk=%d q_col0=%d k_col0=%d ld_out=%d ldvt=%d", p.ld_qk, p.q_col0, p.k_col0, p.ld_out, p.ldvt);
    const dim3 grid((p.max_len + 15) / 16, std::min(p.n_seq, 65535), p.heads);
    const float scale_log2 = 1.4426950408889634f * p.scale;
    TtProfScope prof(TT_K_ATTENTION, st);
    if (p.head_dim == 64)
        hipLaunchKernelGGL(keylimit_attention_kernel<64>, grid, dim3(64), 0, st, p.qk, p.ld_qk, p.q_col0, p.k_col0, p.vt, p.ldvt, p.out,
                           p.ld_out, p.seq_start, p.seq_len, key_len, p.n_seq, scale_log2);
    else
        hipLaunchKernelGGL(keylimit_attention_kernel<32>, grid, dim3(64), 0, st, p.qk, p.ld_qk, p.q_col0, p.k_col0, p.vt, p.ldvt, p.out,
                           p.ld_out, p.seq_start, p.seq_len, key_len, p.n_seq, scale_log2);
    TT_CHECK_LAUNCH();
    return TT_OK;
}

extern "C" {

int tt_maxsim(const void* q_vecs, const int32_t* q_start, const int32_t* q_len, int n_q, const void* d_vecs, const int64_t* d_start,
              const int32_t* d_len, const int32_t* cand, int n_cand, int dim, float* scores, void* stream) {
    if (dim <= 0 || dim % 32 || dim > kMaxDim) {
        tt_set_error("tt_maxsim: dim=%d must be a multiple of 32 and <= %d", dim, kMaxDim);
        return TT_E_UNSUPPORTED;
    }
    TT_CHECK_ARG(n_q >= 0 && n_cand >= 0 && n_q <= 65535, "n_q=%d n_cand=%d", n_q, n_cand);
    if (n_q == 0 || n_cand == 0) return TT_OK;
    TT_CHECK_ARG(q_vecs && q_start && q_len && d_vecs && d_start && d_len && scores, "null pointer");
    hipStream_t st = (hipStream_t)stream;
    const uint16_t* q = (const uint16_t*)q_vecs;
    const uint16_t* d = (const uint16_t*)d_vecs;
    TtProfScope prof(TT_K_ROWOPS, st);
    switch (dim) {
        case 32: maxsim_launch<32>(q, q_start, q_len, n_q, d, d_start, d_len, cand, n_cand, scores, st); break;
        case 64: maxsim_launch<64>(q, q_start, q_len, n_q, d, d_start, d_len, cand, n_cand, scores, st); break;
        case 96: maxsim_launch<96>(q, q_start, q_len, n_q, d, d_start, d_len, cand, n_cand, scores, st); break;
        default: maxsim_launch<128>(q, q_start, q_len, n_q, d, d_start, d_len, cand, n_cand, scores, st); break;
    }
    TT_CHECK_LAUNCH();
    return TT_OK;
}

#if !TT_F16
size_t tt_maxsim_scan_workspace_bytes(int64_t n_docs, int n_q) {
    if (n_docs < 0 || n_q <= 0) return 0;
    const int64_t stride = (n_docs + 31) / 32 * 32;
    return tt_align_up((size_t)n_q * stride * sizeof(float), 256);
}
#endif

int tt_maxsim_scan_topk(const void* q_vecs, const int32_t* q_start, const int32_t* q_len, int n_q, const void* d_vecs,
                        const int64_t* d_start, const int32_t* d_len, const uint8_t* alive, int64_t n_docs, int dim, int k,
                        float* out_scores, int32_t* out_idx, void* workspace, size_t workspace_bytes, void* stream) {
    const char* name = kF16 ? "tt_maxsim_scan_topk_f16" : "tt_maxsim_scan_topk";
    if (dim <= 0 || dim % 32 || dim > kMaxDim) {
        tt_set_error("%s: dim=%d must be a multiple of 32 and <= %d", name, dim, kMaxDim);
        return TT_E_UNSUPPORTED;
    }
    if (n_q < 1 || n_q > kScanMaxQueries || k < 1 || k > 1024) {
        tt_set_error("%s: n_q=%d (1 .. %d), k=%d (1 .. 1024)", name, n_q, kScanMaxQueries, k);
        return TT_E_UNSUPPORTED;
    }
    TT_CHECK_ARG(n_docs >= 0 && n_docs <= INT_MAX, "%s: n_docs=%lld", name, (long long)n_docs);
    TT_CHECK_ARG(out_scores && out_idx, "%s: null output", name);
    hipStream_t st = (hipStream_t)stream;
    if (n_docs == 0) {
        const int64_t n = (int64_t)n_q * k;
        hipLaunchKernelGGL(maxsim_scan_pad_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, out_scores, out_idx, n);
        TT_CHECK_LAUNCH();
        return TT_OK;
    }
    TT_CHECK_ARG(q_vecs && q_start && q_len && d_vecs && d_start && d_len, "%s: null pointer", name);
    const size_t need = tt_maxsim_scan_workspace_bytes(n_docs, n_q);
    if (!workspace || workspace_bytes < need) {
        tt_set_error("%s: workspace %zu < required %zu bytes", name, workspace_bytes, need);
        return TT_E_WORKSPACE;
    }
    const int cus = tt_cu_count_cached();
    TT_CHECK_ARG(cus > 0, "%s: no device", name);
    const int64_t stride = (n_docs + 31) / 32 * 32;
    float* dense = (float*)workspace;
    // a persistent grid: kScanWgPerCu workgroups per compute unit, never more than there are chunks for their waves
    const int64_t chunks = (n_docs + kScanChunk - 1) / kScanChunk;
    const int grid = (int)std::min<int64_t>((int64_t)cus * kScanWgPerCu, (chunks + kScanWaves - 1) / kScanWaves);
    const uint16_t* q = (const uint16_t*)q_vecs;
    const uint16_t* d = (const uint16_t*)d_vecs;
    {
        TtProfScope prof(TT_K_ROWOPS, st);
#define TT_MAXSIM_SCAN(D)                                                                                                        \
    hipLaunchKernelGGL(maxsim_scan_kernel<D>, dim3(grid), dim3(64 * kScanWaves), 0, st, q, q_start, q_len, n_q, d, d_start, d_len, \
                       alive, (int)n_docs, dense, stride)
        switch (dim) {
            case 32: TT_MAXSIM_SCAN(32); break;
            case 64: TT_MAXSIM_SCAN(64); break;
            case 96: TT_MAXSIM_SCAN(96); break;
            default: TT_MAXSIM_SCAN(128); break;
        }
#undef TT_MAXSIM_SCAN
        TT_CHECK_LAUNCH();
    }
    // the lexical scan's selection: a dead document's slot holds NaN, which the selection's key rejects
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

int tt_colbert_project(const void* hidden, int n_rows, int H, const void* w, int dim, const int32_t* rows, int n_out, void* out,
                       void* stream) {
    if (H <= 0 || H % 128 || H > 1024) {
        tt_set_error("tt_colbert_project: hidden=%d must be a multiple of 128 and <= 1024", H);
        return TT_E_UNSUPPORTED;
    }
    if (dim <= 0 || dim % 32 || dim > kMaxDim) {
        tt_set_error("tt_colbert_project: dim=%d must be a multiple of 32 and <= %d", dim, kMaxDim);
        return TT_E_UNSUPPORTED;
    }
    TT_CHECK_ARG(n_rows > 0 && n_out >= 0, "n_rows=%d n_out=%d", n_rows, n_out);
    if (n_out == 0) return TT_OK;
    TT_CHECK_ARG(hidden && w && rows && out, "null pointer");
    hipStream_t st = (hipStream_t)stream;
    TtProfScope prof(TT_K_ROWOPS, st);
    hipLaunchKernelGGL(colbert_project_kernel, dim3((n_out + 15) / 16), dim3(64 * kProjWaves), 0, st, (const uint16_t*)hidden, n_rows, H,
                       (const uint16_t*)w, dim, rows, n_out, (uint16_t*)out);
    TT_CHECK_LAUNCH();
    return TT_OK;
}

int tt_attention_keylimit(const void* qk, int ld_qk, int q_col0, int k_col0, const void* vt, int ldvt, void* out, int ld_out,
                          const int32_t* seq_start, const int32_t* seq_len, const int32_t* key_len, int n_seq, int heads, int head_dim,
                          int max_len, void* stream) {
    TT_CHECK_ARG(qk && vt && out && seq_start && seq_len && key_len, "null pointer");
    AttnParams a{};
    a.qk = (const uint16_t*)qk; a.ld_qk = ld_qk; a.q_col0 = q_col0; a.k_col0 = k_col0;
    a.vt = (const uint16_t*)vt; a.ldvt = ldvt; a.out = (uint16_t*)out; a.ld_out = ld_out;
    a.seq_start = seq_start; a.seq_len = seq_len; a.n_seq = n_seq; a.heads = heads; a.head_dim = head_dim;
    a.max_len = max_len; a.scale = 1.0f / sqrtf((float)(head_dim > 0 ? head_dim : 1));
    return tt_attention_keylimit_launch(a, key_len, (hipStream_t)stream);
}

}  // extern "C"
