// Which attention kernel a launch takes, and on what grid: the decision of attention.hip's launchers as pure host functions.  No HIP in
// here -- tests/test_attention_plan_host.py compiles this header with the host compiler and checks the dispatch on a CPU (every kernel
// form gives the same bits by design, so a GPU test cannot see a batch move from the four-wave to the eight-wave kernel).
#pragma once
#include <stddef.h>

// A/B switches of kept decisions (diagnostic library: TT_ATT_WAVES / TT_ATT_LAZY / TT_ATT_IO, read in attention.hip; the product library
// runs these defaults).  A row's bits do not depend on any of them.
struct AttnSwitches {
    int waves = 0;            // WAVES=4|8: that many waves per workgroup instead of the measured rule (0 = the rule)
    float lazy = 8.f;         // LAZY: log2 slack of the running softmax reference (0 = classic running maximum; not part of the plan)
    int line_stores = -1;     // IO=0: the 8-byte context stores even where whole rows could be written (-1, 1 = the rule)
};

struct AttnPlan {
    int waves;                // 32-row query blocks per workgroup: 4 or 8
    bool line_stores;         // the context leaves in whole rows (attention_kernel's LINE_STORES)
    int n_qt;                 // query tiles (workgroups) per (sequence, head)
    long long workgroups;     // heads * n_seq * n_qt: the launcher refuses more than 0x7FFFFFFF
};

// The plan of ONE launch of a shape the launcher accepts (it validates first; a refused shape has no meaningful plan).
// total_rows: token rows of the batch, <= 0 = unknown.  out_aligned16: the output base is 16-byte aligned.
inline AttnPlan attention_plan(int head_dim, int heads, int n_seq, int max_len, long long total_rows, int ld_qk, int ld_out,
                               bool out_scales, bool out_aligned16, const AttnSwitches& sw) {
    // Waves (32-row query blocks) per workgroup, chosen per batch from B = ceil(max_len / 32) (measured at 1600 sequences x 16 heads,
    // profiles/r04_attention_eight_waves_ab.log): EIGHT waves (256 rows: half the K / V copies and barriers per query row, two waves per
    // SIMD like two four-wave workgroups) win where the last workgroup of a sequence is at least five-eighths full -- B = 5..8 (130
    // tokens +32 %, 160 +26 %, 200 +13 %) and B = 13..16 (420 +6 %, 512 +5 %) -- and lose where it is nearly empty (B = 9, 10: 258 /
    // 292 / 320 tokens -20...-23 %).  32-wide heads always take four waves.
    int waves = 4;
    if (head_dim == 64) {
        const int B = (int)(((long long)max_len + 31) / 32), r8 = B % 8;
        if (sw.waves == 4 || sw.waves == 8) waves = sw.waves;
        // ... and only for batches of SIMILAR lengths (rerank pairs, length-sorted embedding windows): a short sequence in an
        // eight-wave launch is one workgroup with mostly idle waves (64 tokens: +20 %), so the mean length must be near max_len
        // (rows are padded to 8 per sequence; unknown total: the caller is a test or a tool with uniform lengths)
        else if (B >= 5 && (r8 == 0 || r8 >= 5) && (total_rows <= 0 || total_rows * 10 >= (long long)n_seq * max_len * 7)) waves = 8;
        // The four-wave kernel steps from a wave's first K piece to its next by toggling bit 6 of the lane's byte offset (kvoff0 ^ 64),
        // which is the chunk swizzle only while the K row stride is a multiple of 128 bytes.  Any other stride (found by
        // tests/test_attention_io_gpu.py: every sequence of more than one key tile came out wrong) takes the eight-wave kernel, one K
        // piece per wave: the same bits.  (The package's own strides are multiples of heads x 64.)
        if (ld_qk % 64) waves = 8;
    }
    const int n_qt = (int)(((long long)max_len + 32 * waves - 1) / (32 * waves));
    // Whole-row context stores need 16-byte aligned rows; the f16c planes (out_scales) keep their own stores.
    const bool line_stores = !out_scales && ld_out % 8 == 0 && out_aligned16 && sw.line_stores != 0;
    return {waves, line_stores, n_qt, (long long)heads * n_seq * n_qt};
}

// CLS-only kernel: one fp32 score per key of the aligned key frame (up to 7 slots in front of the sequence), rounded up to 8.  The
// launcher refuses more than 160 KiB.
inline size_t attention_cls_lds_bytes(int max_len) { return (size_t)(((long long)max_len + 14) / 8 * 8) * sizeof(float); }
