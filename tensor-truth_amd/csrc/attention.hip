// Variable-length bidirectional self-attention (flash-style, online softmax), gfx950 MFMA.
//
//   ctx[t][h*dh + d] = sum_k softmax_k(Q[t].K[k] / sqrt(dh)) V[k][d]   over the keys of t's sequence
//
// Replaces the scaled-dot-product attention inside the reference's XLM-R / BERT encoder
// layers (additive -inf key-padding mask == attending only to the sequence's own tokens
// in the packed varlen layout).
//
// One workgroup = 4 waves (one per SIMD) = 128 query rows of one (sequence, head), or 8 waves = 256 rows where
// attention_plan.h's measured rule says so; keys stream through LDS in tiles of 64, staged by
// LDS-DMA (global_load_lds_dwordx4) into two buffers: the copies of tile t+1 are in flight while tile t is
// computed and there is ONE barrier per tile.  Both products run "swapped" on v_mfma_f32_32x32x16_bf16 so
// that the QUERY sits on the lane for the whole kernel:
//   S^T[key][q] = K . Q^T      A = K fragment (ds_read_b128, XOR-swizzled rows), B = Q fragment (registers)
//   O^T[d][q]  += V^T . P^T    A = V^T fragment (one ds_read_b128), B = the S^T accumulator itself,
//                              converted to bf16 in place
// so the softmax row statistics are lane-local (one cross-half exchange per tile) and P never goes through
// LDS.  The K rows are fed to the first product in a permuted order (row bits 2 and 3 swapped) so that the
// eight accumulator registers a lane converts into one P fragment are eight CONSECUTIVE keys: exactly one
// 16-byte piece of the token-blocked V copy the QKV GEMM epilogue wrote (V8: [token/8][feature][8]), which
// therefore goes global -> LDS -> MFMA operand without any transposition or padding.
#include "common.h"
#include "attention_plan.h"
#include "encoder.h"
#include "f16c.h"

namespace {

constexpr int kKTile = 64;    // keys per LDS tile

typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
// LDS reads hidden from the compiler's LDS-DMA tracking (it would put s_waitcnt vmcnt(0) in front of every
// ds_read while the next tile's copies are in flight); lds_wait4 is the matching lgkmcnt(0).
template <int OFF>
__device__ __forceinline__ u32x4 lds_read128_async(uint32_t addr) {
    u32x4 r;
    asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(r) : "v"(addr), "n"(OFF));
    return r;
}
// wait until at most N LDS reads of this wave are still in flight (they return in order)
template <int N>
__device__ __forceinline__ void lds_wait4n(u32x4& a, u32x4& b, u32x4& c, u32x4& d) {
    asm volatile("s_waitcnt lgkmcnt(%4)" : "+v"(a), "+v"(b), "+v"(c), "+v"(d) : "n"(N));
}
template <int N>
__device__ __forceinline__ void lds_wait2n(u32x4& a, u32x4& b) {
    asm volatile("s_waitcnt lgkmcnt(%2)" : "+v"(a), "+v"(b) : "n"(N));
}
typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ void lds_write64_async(uint32_t addr, uint2 v) {
    const u32x2 d = u32x2{v.x, v.y};
    asm volatile("ds_write_b64 %0, %1" :: "v"(addr), "v"(d) : "memory");
}

// NW: waves = 32-row query blocks per workgroup.  4, or 8 (256 rows) where a sequence's last workgroup stays mostly full
// (attention_plan.h: the measured rule).  A row's arithmetic does not depend on NW.
// LINE_STORES: how the context leaves.  true: the context block of a wave (32 rows x DH) is transposed through the wave's slice of
// the dead K / V buffers and leaves in whole rows: DH = 64: four global_store_dwordx4 per wave, each eight full 128-byte lines (eight
// lanes per row); DH = 32: two, each sixteen 64-byte rows.  false: a lane writes its own row in 8-byte pieces -- kept for the f16c
// planes and for outputs that are not 16-byte aligned (attention_plan.h).  Same bits either way.
template <int DH, int NW, bool LINE_STORES>
__global__ __launch_bounds__(64 * NW, 4) void attention_kernel(AttnParams p) {
    constexpr int RB = DH * 2;              // bytes per K row
    constexpr int CH = RB / 16;             // 16-B chunks per K row
    constexpr int RPB = 256 / RB;           // K rows per 256-B bank row
    constexpr int KS = DH / 16;             // k-steps of Q.K
    constexpr int DT = DH / 32;             // 32-row d tiles of O^T
    constexpr int NPK = kKTile * RB / 1024; // 1-KiB copy pieces of a K tile
    constexpr int NPV = 8 * DH * 16 / 1024; // ... of a V tile (8 token groups x DH features x 16 B)
    constexpr int KPW = NPK / NW, VPW = NPV / NW;   // pieces per wave: NW = 4: 2 + 2 (dh 64), 1 + 1 (dh 32); NW = 8: 1 + 1
    static_assert(NPK % NW == 0 && NPV % NW == 0, "every wave copies the same number of pieces");
    constexpr int BUF = (NPK + NPV) * 1024;
    // Two buffers: tile kt + 1 is copied while tile kt is computed.  (Three -- copies two tiles ahead, a copy needs about 3 us
    // to land under load and a tile 2-2.5 us to compute -- cost a workgroup per CU at 48 KiB each and measured 20 % slower,
    // 1.62 vs 1.35 ms at 1600 x 292 tokens and at every other length tried: resident waves hide more than the deeper prefetch.)
    __shared__ __attribute__((aligned(1024))) char lds[2 * BUF];

    // Workgroup -> (query tile, head, sequence), the tile fastest.  The grid is exactly heads * n_seq * n_qt workgroups (the
    // launcher's plan), so every pair decoded here exists; a tile past the end of a SHORT sequence leaves below.  (In this order the
    // tiles of a pair are dealt to different XCDs and each L2 fetches the pair's K / V again; an XCD-aware order that avoids it
    // measured neutral end to end and is not kept: DESIGN_HISTORY.md section 4.4, profiles/r06_attention_xcd_ab.log.)
    const int L = blockIdx.x, qt = L % p.n_qt, pair = L / p.n_qt;
    const int head = pair % p.heads, seq = pair / p.heads;
    const int len = p.seq_len[seq];
    if (qt * 32 * NW >= len) return;
    const int t0 = p.seq_start[seq];
    // Sequences may start at any row.  Keys are walked in the ALIGNED frame of the V8 token groups: aligned key ka is
    // global row t0a + ka, t0a = t0 rounded down to 8; the off = t0 - t0a rows in front of the sequence (the tail of its
    // predecessor) and everything from off + len on are masked.
    const int t0a = t0 & ~7, off = t0 - t0a, alen = off + len;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int ql = lane & 31, hh = lane >> 5;
    const uint32_t lds0 = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) char*)lds;

    // ---- Q fragments (B operand), straight from global ---------------------------------
    const int q_row = (qt * NW + wave) * 32 + ql;         // row inside the sequence
    const int q_row_c = q_row < len ? q_row : len - 1;     // clamp: result discarded
    const uint16_t* qp = p.qk + (size_t)(t0 + q_row_c) * p.ld_qk + p.q_col0 + head * DH + hh * 8;
    ex8 qf[KS];
#pragma unroll
    for (int s = 0; s < KS; ++s) qf[s] = *reinterpret_cast<const ex8*>(qp + s * 16);

    const int n_kt = (alen + kKTile - 1) / kKTile;
    const int n_g8 = (alen + 7) >> 3;
    // ---- staging: wave w copies K pieces w*KPW.. and V pieces w*VPW.. of each tile.  Per-lane row / token-group
    // indices are loop constants; rows / groups beyond the sequence are clamped to its last one (finite values;
    // their probabilities are 0) -- only the last tile can need that.
    const uint16_t* kbase = p.qk + (size_t)t0a * p.ld_qk + p.k_col0 + head * DH;
    const uint16_t* vbase = p.vt + (size_t)(t0a >> 3) * p.ldvt + (size_t)head * DH * 8;
    // Copies in the SGPR-base form (wave-uniform 64-bit base + per-lane 32-bit byte offset, as the GEMM's glds16), with ONE
    // per-lane offset register per operand.  History: through the builtin every piece carried a per-lane 64-bit address
    // (v_mad_i64_i32 + v_lshl_add_u64 and a VGPR pair per piece and tile); with per-piece offset arrays kept across the loop
    // the kernel, which sits at its 128-VGPR cap, spilled two of them and reloaded them INSIDE the key loop behind an
    // s_waitcnt vmcnt(0) -- a drain of the copy queue per tile, 6 % of the bench shape's time.  Piece i of a wave is piece 0
    // moved by 64 / CH rows (K) or 64 / DH token groups (V): a scalar step of the BASE; the K swizzle (r / RPB) & (CH - 1)
    // advances by 4 per piece, i.e. toggles bit 2 of the chunk index (byte offset ^ 64) for odd i when CH = 8.
    constexpr int kRowsPerPiece = 64 / CH, kGroupsPerPiece = 64 / DH > 0 ? 64 / DH : 1;
    static_assert(KPW == 1 || CH == 8, "piece-to-piece swizzle step is written for 128-byte K rows");
    static_assert(VPW == 1 || DH == 64, "one token group per V piece");
    const uint32_t lds_base = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) char*)lds;
    uint32_t kvoff0, vvoff0;             // byte offsets of this lane inside the wave's piece 0 of an unclamped tile
    {
        const int e = wave * KPW * 64 + lane, r = e / CH, pos = e % CH;
        kvoff0 = ((uint32_t)r * (uint32_t)p.ld_qk + (uint32_t)((pos ^ ((r / RPB) & (CH - 1))) << 3)) * 2u;
        const int ev = wave * VPW * 64 + lane;
        vvoff0 = ((uint32_t)(ev / DH) * (uint32_t)p.ldvt + (uint32_t)((ev % DH) * 8)) * 2u;
    }
    auto sbase = [](const void* ptr) {      // keep a wave-uniform pointer in SGPRs
        const unsigned long long b = reinterpret_cast<unsigned long long>(ptr);
        const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)b), hi = __builtin_amdgcn_readfirstlane((unsigned)(b >> 32));
        return reinterpret_cast<const char*>(((unsigned long long)hi << 32) | lo);
    };
    auto glds16 = [](const char* base, uint32_t voff, uint32_t lds_addr) {
        asm volatile("s_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %0, %1" ::"v"(voff), "s"(base), "s"(lds_addr) : "memory", "m0");
    };
    auto issue_tile = [&](int kt) {
        const uint32_t buf = lds_base + (uint32_t)(kt & 1) * BUF;
        const bool clamp = (kt + 1) * kKTile > alen || (kt == 0 && off != 0);   // wave-uniform
        if (!clamp) {
#pragma unroll
            for (int i = 0; i < KPW; ++i)
                glds16(sbase(kbase + ((size_t)kt * kKTile + i * kRowsPerPiece) * p.ld_qk), (i & 1) ? (kvoff0 ^ 64u) : kvoff0,
                       buf + (uint32_t)(wave * KPW + i) * 1024u);
#pragma unroll
            for (int i = 0; i < VPW; ++i)
                glds16(sbase(vbase + ((size_t)kt * 8 + i * kGroupsPerPiece) * p.ldvt), vvoff0, buf + (uint32_t)(NPK + wave * VPW + i) * 1024u);
            return;
        }
        // first / last tile: rows / token groups outside the sequence are clamped to its nearest one (finite values; their
        // probabilities are 0).  The per-lane indices are recomputed here instead of living in registers across the loop.
        const char* kb = sbase(kbase);
        const char* vb = sbase(vbase);
        int lane_c = lane;
        asm volatile("" : "+v"(lane_c));
        auto clamped_k = [&](int piece) {
            const int e = piece * 64 + lane_c, r = e / CH, pos = e % CH;
            int row = kt * kKTile + r;
            row = row < off ? off : (row < alen ? row : alen - 1);               // rows of this sequence only
            glds16(kb, ((uint32_t)row * (uint32_t)p.ld_qk + (uint32_t)((pos ^ ((r / RPB) & (CH - 1))) << 3)) * 2u,
                   buf + (uint32_t)piece * 1024u);
        };
        auto clamped_v = [&](int piece) {
            const int e = piece * 64 + lane_c;
            int g8 = kt * 8 + e / DH;
            g8 = g8 < n_g8 ? g8 : n_g8 - 1;
            glds16(vb, ((uint32_t)g8 * (uint32_t)p.ldvt + (uint32_t)((e % DH) * 8)) * 2u, buf + (uint32_t)(NPK + piece) * 1024u);
        };
#pragma unroll
        for (int i = 0; i < KPW; ++i) clamped_k(wave * KPW + i);
#pragma unroll
        for (int i = 0; i < VPW; ++i) clamped_v(wave * VPW + i);
    };

    f32x16 acc_o[DT];
#pragma unroll
    for (int d = 0; d < DT; ++d)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc_o[d][r] = 0.f;
    float m_run = -__builtin_inff();
    float l_run = 0.f;
    const float sc = p.scale * 1.4426950408889634f;  // fold log2(e): softmax via exp2
    const bool wave_active = (qt * NW + wave) * 32 < len;      // wave-uniform; idle waves only help staging

    // per-lane LDS offsets: K row perm(ql) (bits 2 and 3 of the row swapped), chunk (2s + hh) ^ swizzle(row)
    const int krow = (ql & 0x13) | ((ql & 4) << 1) | ((ql & 8) >> 1);
    uint32_t koff[KS];
#pragma unroll
    for (int s = 0; s < KS; ++s) koff[s] = lds0 + krow * RB + (((2 * s + hh) ^ ((krow / RPB) & (CH - 1))) << 4);
    const uint32_t voff = lds0 + NPK * 1024 + (hh * DH + ql) * 16;    // + (4j + 2 s2) * DH*16 + 32*dt*16

    issue_tile(0);
    for (int kt = 0; kt < n_kt; ++kt) {
        const int k0 = kt * kKTile;
        // This wave's pieces of tile kt have landed.  As the BUILTIN, not inline asm: the waitcnt pass must see a vmcnt(0)
        // on every path into the loop -- the Q fragments are ordinary global loads of the prologue, and otherwise it protects
        // their first use in EVERY iteration with s_waitcnt vmcnt(3..0), which at run time also counts the copies of tile
        // kt + 1 issued a moment earlier: a full drain of the prefetch per tile (the double buffer was single-buffered in
        // effect; -2...4 % on top of the spill fix above).
        __builtin_amdgcn_s_waitcnt(0x0F70);
        asm volatile("" ::: "memory");
        __builtin_amdgcn_sched_barrier(0);
        __builtin_amdgcn_s_barrier();                       // ... everyone's; and tile kt-1 is no longer read
        __builtin_amdgcn_sched_barrier(0);
        if (kt + 1 < n_kt) issue_tile(kt + 1);
        if (!wave_active) continue;
        const uint32_t bufo = (kt & 1) * BUF;

        // ---- S^T = K . Q^T for two 32-key tiles -------------------------------------------------
        f32x16 acc_s[2];
        {
            u32x4 kf[2][4];
            uint32_t ka[KS];
#pragma unroll
            for (int s = 0; s < KS; ++s) ka[s] = koff[s] + bufo;
#pragma unroll
            for (int s = 0; s < KS; ++s) kf[0][s] = lds_read128_async<0>(ka[s]);
#pragma unroll
            for (int s = 0; s < KS; ++s) kf[1][s] = lds_read128_async<32 * RB>(ka[s]);
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                if (j == 0) {
                    if constexpr (KS == 4) lds_wait4n<KS>(kf[0][0], kf[0][1], kf[0][2], kf[0][3]);
                    else lds_wait2n<KS>(kf[0][0], kf[0][1]);
                } else {
                    if constexpr (KS == 4) lds_wait4n<0>(kf[1][0], kf[1][1], kf[1][2], kf[1][3]);
                    else lds_wait2n<0>(kf[1][0], kf[1][1]);
                }
#pragma unroll
                for (int r = 0; r < 16; ++r) acc_s[j][r] = 0.f;
#pragma unroll
                for (int s = 0; s < KS; ++s)
                    acc_s[j] = TT_MFMA_32x32x16(__builtin_bit_cast(ex8, kf[j][s]), qf[s], acc_s[j]);
            }
        }
        // V fragments of the first 32 keys: in flight during the softmax
        u32x4 vf[2][2];   // [s2][dt]
        const uint32_t vaddr = voff + bufo;
        vf[0][0] = lds_read128_async<0>(vaddr);
        if constexpr (DT == 2) vf[0][1] = lds_read128_async<512>(vaddr);
        vf[1][0] = lds_read128_async<2 * DH * 16>(vaddr);
        if constexpr (DT == 2) vf[1][1] = lds_read128_async<2 * DH * 16 + 512>(vaddr);

        // ---- mask the tail, running max, exponentials --------------------------------------------
        // The softmax scale (and log2 e) is folded into one FMA per score: p = 2^(s*sc - m), with m
        // tracked in the scaled domain; v_exp_f32 is used raw (arguments are <= 0, a result that
        // underflows is 0 either way), the libm exp2f wraps it in 5 more instructions per value.
        // Register r of tile j is key k0 + 32 j + 16 (r>>3) + 8 hh + (r & 7)  (permuted K rows).
        if (kt == 0 && off != 0) {   // wave-uniform: the first off (< 8) aligned keys belong to the previous sequence
            if (hh == 0) {
#pragma unroll
                for (int r = 0; r < 8; ++r)
                    if (r < off) acc_s[0][r] = -__builtin_inff();
            }
        }
        if (k0 + kKTile > alen) {   // wave-uniform; one compare per value against a lane constant, no index arithmetic
            const int lim = alen - k0 - 8 * hh;   // register r of tile j is masked iff 32 j + 16 (r>>3) + (r&7) >= lim
#pragma unroll
            for (int j = 0; j < 2; ++j)
#pragma unroll
                for (int r = 0; r < 16; ++r)
                    if (32 * j + 16 * (r >> 3) + (r & 7) >= lim) acc_s[j][r] = -__builtin_inff();
        }
        float mx = -__builtin_inff();
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) mx = fmaxf(mx, acc_s[j][r]);
        mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
        // Lazy running maximum: m only moves when a tile's maximum exceeds it by more than 2^lazy (p.lazy = 8; it is a scaling
        // reference, not a bound: probabilities up to 2^lazy are exact in fp32 sums and keep their relative precision
        // as bf16 MFMA operands, and the final division by l uses the same reference).  After the first tile the
        // reference almost never moves, alpha is 1 on every lane and the 32-register rescale of O is skipped.
        const float mt = mx * sc;
        const float m_new = (mt > m_run + p.lazy) ? mt : m_run;       // first tile: m_run = -inf -> mt (finite: >= 1 valid key)
        const float alpha = __builtin_amdgcn_exp2f(m_run - m_new);   // first tile: 2^-inf = 0
        m_run = m_new;
        f32x2 psum2 = f32x2{0.f, 0.f};
        const f32x2 sc2 = f32x2{sc, sc}, mn2 = f32x2{m_new, m_new};
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 16; r += 2) {
                const f32x2 t = f32x2{acc_s[j][r], acc_s[j][r + 1]} * sc2 - mn2;
                const f32x2 e = f32x2{__builtin_amdgcn_exp2f(t.x), __builtin_amdgcn_exp2f(t.y)};
                acc_s[j][r] = e.x;
                acc_s[j][r + 1] = e.y;
                psum2 += e;
            }
        l_run = l_run * alpha + (psum2.x + psum2.y);
        if (kt > 0 && !__all(alpha == 1.0f)) {   // (first tile: O is still zero) the running max rarely moves later
#pragma unroll
            for (int d = 0; d < DT; ++d)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc_o[d][r] *= alpha;
        }

        // ---- O^T += V^T . P^T ----------------------------------------------------------------------
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            if constexpr (DT == 2) lds_wait4n<0>(vf[0][0], vf[0][1], vf[1][0], vf[1][1]);
            else lds_wait2n<0>(vf[0][0], vf[1][0]);
            ex8 va[2][2];
#pragma unroll
            for (int s2 = 0; s2 < 2; ++s2)
#pragma unroll
                for (int d = 0; d < DT; ++d) va[s2][d] = __builtin_bit_cast(ex8, vf[s2][d]);
            if (j == 0) {   // next 32 keys' fragments, in flight during these MFMAs
                vf[0][0] = lds_read128_async<4 * DH * 16>(vaddr);
                if constexpr (DT == 2) vf[0][1] = lds_read128_async<4 * DH * 16 + 512>(vaddr);
                vf[1][0] = lds_read128_async<6 * DH * 16>(vaddr);
                if constexpr (DT == 2) vf[1][1] = lds_read128_async<6 * DH * 16 + 512>(vaddr);
            }
#pragma unroll
            for (int s2 = 0; s2 < 2; ++s2) {
                uint4 pb;
                pb.x = pack_e2_inrange(acc_s[j][8 * s2 + 0], acc_s[j][8 * s2 + 1]);
                pb.y = pack_e2_inrange(acc_s[j][8 * s2 + 2], acc_s[j][8 * s2 + 3]);
                pb.z = pack_e2_inrange(acc_s[j][8 * s2 + 4], acc_s[j][8 * s2 + 5]);
                pb.w = pack_e2_inrange(acc_s[j][8 * s2 + 6], acc_s[j][8 * s2 + 7]);
                const ex8 pf = __builtin_bit_cast(ex8, pb);
#pragma unroll
                for (int d = 0; d < DT; ++d)
                    acc_o[d] = TT_MFMA_32x32x16(va[s2][d], pf, acc_o[d]);
            }
        }
    }

    // ---- normalise and store: lane = query row, registers = 4 consecutive d ------------------
    const float l_tot = l_run + __shfl_xor(l_run, 32, 64);
    const float inv = 1.0f / l_tot;
    if (q_row < len) {
        if (p.out_scales) {
            // f16c: c-planes.  A scale block = 32 consecutive columns = one d tile of this head: this lane's 16 values and those
            // of the lane holding the row's other column quads (hh ^ 1: same q_row, so both are inside this branch).
            char* orow = reinterpret_cast<char*>(p.out) + (size_t)(t0 + q_row) * p.ld_out * 2;
            const int W = p.out_width, nks = W >> 7;
#pragma unroll
            for (int d = 0; d < DT; ++d) {
                float y[16];
                float amax = 0.f;
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    y[r] = acc_o[d][r] * inv;
                    asm("" : "+v"(y[r]));            // opaque: no fusing of "* inv" into the "y - hi" of the split
                    amax = fmaxf(amax, fabsf(y[r]));
                }
                amax = fmaxf(amax, __shfl_xor(amax, 32, 64));
                int sbyte, sh;
                xc_block_scale(amax, sbyte, sh);
                const int col0 = head * DH + 32 * d;
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    uint2 hi;
                    uint32_t x8, l8;
                    xc_split4(y[4 * g + 0], y[4 * g + 1], y[4 * g + 2], y[4 * g + 3], sh, sh + 11, hi, x8, l8);
                    const int col = col0 + 8 * g + 4 * hh;
                    *reinterpret_cast<uint2*>(orow + (size_t)col * 2) = hi;
                    *reinterpret_cast<uint32_t*>(orow + (size_t)2 * W + col) = x8;
                    *reinterpret_cast<uint32_t*>(orow + (size_t)3 * W + col) = l8;
                }
                if (hh == 0) p.out_scales[xc_a_scale_at(t0 + q_row, col0 >> 5, nks)] = (uint8_t)sbyte;
            }
            return;
        }
        if constexpr (!LINE_STORES) {
            uint16_t* op = p.out + (size_t)(t0 + q_row) * p.ld_out + head * DH;
#pragma unroll
            for (int d = 0; d < DT; ++d)
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    uint2 o;
                    o.x = pack_e2(acc_o[d][4 * g + 0] * inv, acc_o[d][4 * g + 1] * inv);
                    o.y = pack_e2(acc_o[d][4 * g + 2] * inv, acc_o[d][4 * g + 3] * inv);
                    *reinterpret_cast<uint2*>(op + 32 * d + 8 * g + 4 * hh) = o;
                }
        }
    }
    if constexpr (LINE_STORES) {
        // ---- whole rows: the wave's block as [32 rows][RB bytes] through LDS, read back CH lanes per row ----------------------
        // (p.out_scales is a kernel argument: every wave of the workgroup takes the same side of this branch)
        if (p.out_scales) return;
        constexpr int RPI = 64 / CH;            // rows per store instruction: 8 whole 128-byte lines (DH 64), 16 rows of 64 B (DH 32)
        constexpr int NI = 32 / RPI;            // store instructions per wave: 4 / 2
        constexpr int RPL = 128 / RB;           // rows per 128 bytes of the slice
        u32x4 t[NI];
        // The K / V buffers are dead once every wave has left the key loop (its last tile's fragments are read, and no copy is in
        // flight: tile n_kt - 1 was waited for at the top of the last iteration).  Idle waves pass the barrier too.
        __builtin_amdgcn_sched_barrier(0);
        __builtin_amdgcn_s_barrier();
        __builtin_amdgcn_sched_barrier(0);
        if (!wave_active) return;
        // wave w's slice: 32 * RB bytes at w * 32 * RB (NW slices fit the two buffers: 8 x 4 KiB = 2 BUF at DH 64).  The 16-byte
        // chunk c of row r sits at chunk c ^ swz(r), swz(r) = (r / RPL) & (CH - 1), as in the GEMM epilogue's staging: the
        // 8-byte writes (16 consecutive rows per lane group) and the 16-byte reads (whole rows) both spread over the banks.
        // (Four-wave slices would also fit the ONE buffer the last tile is not in, which needs no barrier: measured the same,
        // 1.139 against 1.141 ms, profiles/attention_io_gate.log -- not kept.)
        const uint32_t slice = lds0 + (uint32_t)wave * (32 * RB);
        const uint32_t wbase = slice + ql * RB + (((ql / RPL) & (CH - 1)) << 4) + 8 * hh;
#pragma unroll
        for (int d = 0; d < DT; ++d)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                uint2 o;
                o.x = pack_e2(acc_o[d][4 * g + 0] * inv, acc_o[d][4 * g + 1] * inv);
                o.y = pack_e2(acc_o[d][4 * g + 2] * inv, acc_o[d][4 * g + 3] * inv);
                lds_write64_async(wbase ^ (uint32_t)((4 * d + g) << 4), o);      // bits 4.. of the chunk index only: row and half stay
            }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        const int r0 = lane / CH;
        const uint32_t raddr = slice + r0 * RB + (((lane % CH) ^ ((r0 / RPL) & (CH - 1))) << 4);   // + i * RPI * RB: swz(r0 + i RPI) = swz(r0)
        t[0] = lds_read128_async<0>(raddr);
        t[1] = lds_read128_async<RPI * RB>(raddr);
        if constexpr (NI == 4) {
            t[2] = lds_read128_async<2 * RPI * RB>(raddr);
            t[3] = lds_read128_async<3 * RPI * RB>(raddr);
            lds_wait4n<0>(t[0], t[1], t[2], t[3]);
        } else {
            lds_wait2n<0>(t[0], t[1]);
        }
        const int row0 = (qt * NW + wave) * 32 + lane / CH;      // row inside the sequence of this lane's piece in instruction 0
        uint16_t* op = p.out + (size_t)(t0 + row0) * p.ld_out + head * DH + (lane % CH) * 8;
#pragma unroll
        for (int i = 0; i < NI; ++i)
            if (row0 + i * RPI < len) *reinterpret_cast<u32x4*>(op + (size_t)(i * RPI) * p.ld_out) = t[i];
    }
}

// ---- CLS-only attention (last layer): one wave per (sequence, head), the single query row t0 -------------
// Scores with the key on the lane (fp32 dot products, K rows read as 16-B pieces), softmax across the wave,
// then the value sum with the FEATURE on the lane (V8 layout: one 16-B load brings 8 keys of a feature).
// Only the CLS token of the last layer is ever read by the pooling / classification head, so the other
// rows' attention (and their output projection / FFN) is skipped: 1/24 of the encoder's flops.
template <int DH>
__global__ __launch_bounds__(64) void attention_cls_kernel(AttnParams p) {
    extern __shared__ __attribute__((aligned(16))) float probs[];   // [max_len rounded up to 8]
    const int seq = blockIdx.x, head = blockIdx.y, lane = threadIdx.x;
    const int len = p.seq_len[seq], t0 = p.seq_start[seq];
    const int t0a = t0 & ~7, off = t0 - t0a, alen = off + len;   // aligned key frame, as in attention_kernel
    // query row -> registers (every lane holds the whole q: uniform address)
    float q[DH];
    {
        const uint16_t* qp = p.q_rows ? p.q_rows + (size_t)seq * p.ld_q_rows + head * DH : p.qk + (size_t)t0 * p.ld_qk + p.q_col0 + head * DH;
#pragma unroll
        for (int c = 0; c < DH / 8; ++c) {
            const uint4 u = *reinterpret_cast<const uint4*>(qp + c * 8);
            q[c * 8 + 0] = elo(u.x); q[c * 8 + 1] = ehi(u.x);
            q[c * 8 + 2] = elo(u.y); q[c * 8 + 3] = ehi(u.y);
            q[c * 8 + 4] = elo(u.z); q[c * 8 + 5] = ehi(u.z);
            q[c * 8 + 6] = elo(u.w); q[c * 8 + 7] = ehi(u.w);
            if (p.qk_lo_off) {          // f16c: hi + lo planes
                const uint4 l = *reinterpret_cast<const uint4*>(qp + p.qk_lo_off + c * 8);
                q[c * 8 + 0] += elo(l.x); q[c * 8 + 1] += ehi(l.x);
                q[c * 8 + 2] += elo(l.y); q[c * 8 + 3] += ehi(l.y);
                q[c * 8 + 4] += elo(l.z); q[c * 8 + 5] += ehi(l.z);
                q[c * 8 + 6] += elo(l.w); q[c * 8 + 7] += ehi(l.w);
            }
        }
    }
    const float sc = p.scale * 1.4426950408889634f;
    float mx = -__builtin_inff();
    for (int j = off + lane; j < alen; j += 64) {
        const uint16_t* kp = p.qk + (size_t)(t0a + j) * p.ld_qk + p.k_col0 + head * DH;
        float acc = 0.f;
#pragma unroll
        for (int c = 0; c < DH / 8; ++c) {
            const uint4 u = *reinterpret_cast<const uint4*>(kp + c * 8);
            float kf[8] = {elo(u.x), ehi(u.x), elo(u.y), ehi(u.y), elo(u.z), ehi(u.z), elo(u.w), ehi(u.w)};
            if (p.qk_lo_off) {
                const uint4 l = *reinterpret_cast<const uint4*>(kp + p.qk_lo_off + c * 8);
                kf[0] += elo(l.x); kf[1] += ehi(l.x); kf[2] += elo(l.y); kf[3] += ehi(l.y);
                kf[4] += elo(l.z); kf[5] += ehi(l.z); kf[6] += elo(l.w); kf[7] += ehi(l.w);
            }
#pragma unroll
            for (int i = 0; i < 8; ++i) acc = fmaf(q[c * 8 + i], kf[i], acc);
        }
        acc *= sc;
        probs[j] = acc;
        mx = fmaxf(mx, acc);
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) mx = fmaxf(mx, __shfl_xor(mx, off, 64));
    float sum = 0.f;
    const int len8 = (alen + 7) & ~7;
    for (int j = lane; j < len8; j += 64) {
        float e = 0.f;
        if (j >= off && j < alen) e = __builtin_amdgcn_exp2f(probs[j] - mx);
        probs[j] = e;      // aligned keys outside the sequence (same 8-groups) get probability 0
        sum += e;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) sum += __shfl_xor(sum, off, 64);
    __syncthreads();
    // value sum: lane = feature (DH=64) or (feature, key-group parity) (DH=32)
    constexpr int PARTS = 64 / DH;
    const int d = lane % DH, part = lane / DH;
    float o = 0.f;
    for (int g8 = part; g8 * 8 < alen; g8 += PARTS) {
        const uint4 u = *reinterpret_cast<const uint4*>(p.vt + (size_t)(t0a / 8 + g8) * p.ldvt + (size_t)(head * DH + d) * 8);
        const float4 pa = *reinterpret_cast<const float4*>(probs + g8 * 8);
        const float4 pb = *reinterpret_cast<const float4*>(probs + g8 * 8 + 4);
        o = fmaf(pa.x, elo(u.x), o); o = fmaf(pa.y, ehi(u.x), o);
        o = fmaf(pa.z, elo(u.y), o); o = fmaf(pa.w, ehi(u.y), o);
        o = fmaf(pb.x, elo(u.z), o); o = fmaf(pb.y, ehi(u.z), o);
        o = fmaf(pb.z, elo(u.w), o); o = fmaf(pb.w, ehi(u.w), o);
    }
    if constexpr (PARTS == 2) o += __shfl_xor(o, 32, 64);
    if (p.out_scales) {
        // f16c: c-planes (row = sequence index).  DH = 64: lanes 0-31 / 32-63 are the two scale blocks of this head.
        float y = o / sum;
        asm("" : "+v"(y));
        float amax = fabsf(y);
#pragma unroll
        for (int off = 16; off > 0; off >>= 1) amax = fmaxf(amax, __shfl_xor(amax, off, 64));
        int sbyte, sh;
        xc_block_scale(amax, sbyte, sh);
        if (part == 0) {
            const int W = p.out_width, col = head * DH + d;
            char* orow = reinterpret_cast<char*>(p.out) + (size_t)seq * p.ld_out * 2;
            const uint16_t hb = f32_to_ebits(y);
            *reinterpret_cast<uint16_t*>(orow + (size_t)col * 2) = hb;
            orow[(size_t)2 * W + col] = (char)(xc_pack4(xc_sat(ldexpf(y, sh)), 0.f, 0.f, 0.f) & 0xFFu);
            orow[(size_t)3 * W + col] = (char)(xc_pack4(xc_sat(ldexpf(y - ebits_to_f32(hb), sh + 11)), 0.f, 0.f, 0.f) & 0xFFu);
            if ((d & 31) == 0) p.out_scales[xc_a_scale_at(seq, col >> 5, W >> 7)] = (uint8_t)sbyte;
        }
        return;
    }
    if (part == 0) p.out[(size_t)seq * p.ld_out + head * DH + d] = f32_to_ebits(o / sum);
}

// The A/B switches of kept decisions.  The product library runs AttnSwitches' defaults; the diagnostic library reads its environment:
// the wave count and the softmax slack once, TT_ATT_IO at every launch (tools/att_bench alternates it inside one process).
AttnSwitches attention_switches() {
    AttnSwitches sw;
#if TT_DIAG
    const auto env = [](const char* name) -> const char* { const char* e = getenv(name); return e && e[0] ? e : nullptr; };
    static const AttnSwitches once = [&env] {
        AttnSwitches s;
        if (const char* e = env("TT_ATT_WAVES")) s.waves = (int)strtol(e, nullptr, 0);
        if (const char* e = env("TT_ATT_LAZY")) s.lazy = (float)atof(e);
        return s;
    }();
    sw = once;
    if (const char* e = env("TT_ATT_IO")) sw.line_stores = (int)strtol(e, nullptr, 0);
#endif
    return sw;
}

constexpr int kernel_key(int head_dim, int waves, bool line_stores) { return head_dim * 32 + waves * 2 + (line_stores ? 1 : 0); }

template <int DH, int NW, bool LINE_STORES>
void launch_attention(long long workgroups, const AttnParams& q, hipStream_t st) {
    hipLaunchKernelGGL((attention_kernel<DH, NW, LINE_STORES>), dim3((unsigned)workgroups), dim3(64 * NW), 0, st, q);
}

}  // namespace

// validate, plan (attention_plan.h: waves per workgroup, store form, grid), launch
int tt_attention_launch(const AttnParams& p, hipStream_t st) {
    if (p.n_seq <= 0 || p.max_len <= 0) return TT_OK;
    if ((p.ld_qk % 8) || (p.q_col0 % 8) || (p.k_col0 % 8) || (p.ldvt % 8) || (p.ld_out % 4)) {
        tt_set_error("attention: leading dimensions / column offsets must keep 16-byte alignment");
        return TT_E_INVALID;
    }
    if (p.head_dim != 64 && p.head_dim != 32) {
        tt_set_error("attention: head_dim %d not in {32, 64}", p.head_dim);
        return TT_E_UNSUPPORTED;
    }
    const AttnSwitches sw = attention_switches();
    const AttnPlan plan = attention_plan(p.head_dim, p.heads, p.n_seq, p.max_len, p.total_rows, p.ld_qk, p.ld_out, p.out_scales != nullptr,
                                         (reinterpret_cast<uintptr_t>(p.out) & 15) == 0, sw);
    if (plan.workgroups > 0x7FFFFFFFLL) {
        tt_set_error("attention: %lld workgroups exceed the grid limit", plan.workgroups);
        return TT_E_UNSUPPORTED;
    }
    AttnParams q = p;
    q.lazy = sw.lazy;
    q.n_qt = plan.n_qt;
    TtProfScope prof(TT_K_ATTENTION, st);
    switch (kernel_key(p.head_dim, plan.waves, plan.line_stores)) {
        case kernel_key(64, 8, true): launch_attention<64, 8, true>(plan.workgroups, q, st); break;
        case kernel_key(64, 8, false): launch_attention<64, 8, false>(plan.workgroups, q, st); break;
        case kernel_key(64, 4, true): launch_attention<64, 4, true>(plan.workgroups, q, st); break;
        case kernel_key(64, 4, false): launch_attention<64, 4, false>(plan.workgroups, q, st); break;
        case kernel_key(32, 4, true): launch_attention<32, 4, true>(plan.workgroups, q, st); break;
        case kernel_key(32, 4, false): launch_attention<32, 4, false>(plan.workgroups, q, st); break;
        default:      // (32-wide heads with eight waves: no such kernel, and the plan never asks for it)
            tt_set_error("attention: no kernel for head_dim %d with %d waves", p.head_dim, plan.waves);
            return TT_E_UNSUPPORTED;
    }
    TT_CHECK_LAUNCH();
    return TT_OK;
}

// out: [n_seq][ld_out] (row = sequence index, NOT token row)
int tt_attention_cls_launch(const AttnParams& p, hipStream_t st) {
    if (p.n_seq <= 0) return TT_OK;
    const size_t lds = attention_cls_lds_bytes(p.max_len);
    if (lds > 160 * 1024) {
        tt_set_error("attention_cls: max_len %d exceeds the LDS score buffer", p.max_len);
        return TT_E_UNSUPPORTED;
    }
    TtProfScope prof(TT_K_ATTENTION, st);
    const dim3 grid(p.n_seq, p.heads);
    if (p.head_dim == 64) {
        TT_SET_MAX_LDS(attention_cls_kernel<64>, 160 * 1024);
        hipLaunchKernelGGL(attention_cls_kernel<64>, grid, dim3(64), lds, st, p);
    } else if (p.head_dim == 32) {
        TT_SET_MAX_LDS(attention_cls_kernel<32>, 160 * 1024);
        hipLaunchKernelGGL(attention_cls_kernel<32>, grid, dim3(64), lds, st, p);
    } else {
        tt_set_error("attention: head_dim %d not in {32, 64}", p.head_dim);
        return TT_E_UNSUPPORTED;
    }
    TT_CHECK_LAUNCH();
    return TT_OK;
}
