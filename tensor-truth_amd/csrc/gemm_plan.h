// Which kernel a GEMM launch takes, and on what grid: the decision of gemm.hip's launchers as pure host functions.  No HIP in here --
// tests/test_gemm_plan_host.py compiles this header with the host compiler and checks the dispatch on a CPU (all kernel forms
// give the same bits by design, so a GPU test cannot see a shape move from one kernel to another).
#pragma once
#include <stdint.h>

enum { TT_EPI_BIAS = 0, TT_EPI_GELU = 1, TT_EPI_RESIDUAL = 2, TT_EPI_TANH = 3, TT_EPI_QKV = 4,
       TT_EPI_VT = 5 /* internal: whole output stored transposed into vt (the V third of a QKV projection) */,
       TT_EPI_SCAN = 6 /* internal: similarity scan -- A = corpus rows, W = 256 queries, nothing is stored: scores >= the
                          query's threshold (bias[n]) are appended to per-query candidate lists (scan_api.hip) */,
       TT_EPI_RELU = 7 /* max(acc + bias, 0): the up-projection of a ReLU MLP (T5 encoders, t5.hip) */ };

// operand form: plain 16-bit, split planes (GemmParams.x3), e4m3 with row / column scales (.fp8), f16c c-planes (.xc)
enum class GemmForm { Bits16, X3, Fp8, Xc };
enum class GemmKernel { Skinny, Relay, Staged128, TwoStage128, OneTile256, Persistent256 };

// A/B switches of kept decisions (diagnostic library: TT_GEMM_<NAME>, read once in gemm.hip; the product library runs these defaults)
struct GemmSwitches {
    bool skinny = true;       // SKINNY=0: the tile kernels for M <= 256 too
    bool relay = true;        // RELAY=0: split planes on the one-wave skinny kernel
    bool staged = true;       // STAGED=0: no staged 128x128 kernel
    int staged_max = 0;       // STAGED_MAX: 128x128 tiles up to which the staged kernel takes a split-plane GEMM (0 = 2 x CUs)
    int staged16 = 1;         // STAGED16: 0 = not for 16-bit operands, > 1 = that many tiles instead of the CU count
    bool small_v1 = true;     // SMALL_V1=0: 256x256 tiles however few
    int sn = 0;               // SN: column tiles per super-tile (0 = 4)
    bool qkv_split = true;    // QKV_SPLIT=0: one launch with the mixed epilogue
    int nt_store = 1;         // NT_STORE=0: plain stores in the one-tile kernel (not part of the plan)
    bool trace = false;       // TRACE=1: print every 16-bit launch (not part of the plan)
};

struct TileGrid { int sn, sm, blocks; };

// 256x256 tiles.  The 32 tiles an XCD works on at a time are sm row-blocks x sn column-blocks (sm * sn = 32); the A row-blocks of a
// super-tile are shared through that XCD's L2 by its sn column tiles.  blocks = whole super-tiles (a multiple of 8: one range per XCD).
inline TileGrid tile_grid_256(int mt_n, int nt_n, int sn_override) {
    int sn = sn_override > 0 ? sn_override : 4;
    if (sn > nt_n) sn = nt_n;
    if (sn < 1) sn = 1;       // (no column tile: a shape the launchers refuse)
    while (32 % sn) --sn;
    const int sm = 32 / sn;
    const int supers = ((mt_n + sm - 1) / sm) * ((nt_n + sn - 1) / sn);
    return {sn, sm, (supers * sm * sn + 7) / 8 * 8};
}

// 128x128 tiles: super-tiles of 8 row-blocks x up to 8 column-blocks
inline TileGrid tile_grid_128(int mt_n, int nt_n) {
    const int sn = nt_n < 1 ? 1 : nt_n < 8 ? nt_n : 8, sm = 8;
    const int supers = ((mt_n + sm - 1) / sm) * ((nt_n + sn - 1) / sn);
    return {sn, sm, (supers * sm * sn + 7) / 8 * 8};
}

struct GemmPlan {
    GemmKernel kernel;
    TileGrid grid;            // tiled kernels only
    int gx, gy;               // launch grid
};

// The plan of ONE launch of a shape its launcher accepts (the launchers validate; a refused shape has no meaningful plan).
inline GemmPlan gemm_plan(GemmForm form, int epi, int M, int N, int K, int ldc, int ldr, int cu_count, const GemmSwitches& sw) {
    // up to 256 rows (one query's embedding, the CLS tail, the rerank head): a stream of the weight matrix -- one wave per 16 x 16
    // outputs; split planes: a workgroup relaying the accumulator (3 K / 32 steps)
    if ((form == GemmForm::Bits16 || form == GemmForm::X3) && sw.skinny && M > 0 && M <= 256 && M % 64 == 0 && N % 16 == 0 &&
        K % 32 == 0 && (K > 0 || form == GemmForm::X3))
        return {form == GemmForm::X3 && sw.relay ? GemmKernel::Relay : GemmKernel::Skinny, {}, N / 16, M / 16};
    const int mt1 = M / 128, nt1 = N / 128;
    if (form == GemmForm::X3) {
        // a lone caller's rerank (M = 1-8 k rows): up to TWO rounds of 128x128 tiles the staged kernel beats the 256x256 kernel's one
        // round on a fraction of the CUs; beyond that the big tile's half fill per flop wins (profiles/r06_staged_ab.log)
        if (sw.staged && N % 128 == 0 && (long long)mt1 * nt1 <= (sw.staged_max ? sw.staged_max : 2 * cu_count)) {
            const TileGrid g = tile_grid_128(mt1, nt1);
            return {GemmKernel::Staged128, g, g.blocks, 1};
        }
        const TileGrid g = tile_grid_256(M / 256, (N + 255) / 256, sw.sn);       // (N % 64 == 0: the last column tile may be partial)
        return {GemmKernel::OneTile256, g, g.blocks, 1};
    }
    if (form != GemmForm::Bits16) {      // e4m3 (the persistent kernel's fp8 GELU form spills) and f16c: one 256x256 tile per workgroup
        const TileGrid g = tile_grid_256(M / 256, N / 256, sw.sn);
        return {GemmKernel::OneTile256, g, g.blocks, 1};
    }
    // Fewer than half a CU-wave of 256x256 tiles (query embedding, the CLS tail): 128x128 tiles spread the work over 4x the
    // workgroups and are 1.3-1.7x faster there (M = 768: 15 vs 23 us per K = 1024 GEMM).  The V^T epilogue has no 128x128 form.
    const bool small_grid = epi != TT_EPI_VT && (long long)(M / 256) * (N / 256) < 128 && sw.small_v1;
    // (the residual epilogue stages the residual tile as two pseudo K-tiles: needs an even number of K-tiles)
    if (!small_grid && M % 256 == 0 && N % 256 == 0 && ldc % 8 == 0 && (epi != TT_EPI_RESIDUAL || (ldr % 8 == 0 && (K / 64) % 2 == 0))) {
        const TileGrid g = tile_grid_256(M / 256, N / 256, sw.sn);
        // measured (M = 236800): the persistent kernel wins where the epilogue is VALU-heavy (GELU: 1.74 vs 1.78 ms), the
        // one-tile kernel with LDS-transposed full-line stores where it is store-bound (bias: 1.39 vs 1.40 ms)
        const int cus = cu_count / 8 * 8;
        if (epi == TT_EPI_GELU && (K / 64) % 2 == 0 && K / 64 >= 2 && g.blocks > cus && cus >= 8) return {GemmKernel::Persistent256, g, cus, 1};
        return {GemmKernel::OneTile256, g, g.blocks, 1};
    }
    // ONE round of 128x128 tiles (a lone caller's 10-pair rerank): the staged kernel -- M = 3072: attention output 17 -> 15 us,
    // FFN-down 49 -> 42 us; in two rounds the two-stage kernel's two workgroups per CU win
    const TileGrid g = tile_grid_128(mt1, nt1);
    const bool staged = sw.staged16 && sw.staged && (long long)mt1 * nt1 <= (sw.staged16 > 1 ? sw.staged16 : cu_count) && K % 64 == 0;
    return {staged ? GemmKernel::Staged128 : GemmKernel::TwoStage128, g, g.blocks, 1};
}

// 16-bit QKV projection: Q, K columns as a plain bias GEMM and the V columns as un-swapped tiles stored transposed -- two launches, the
// same number of tile rounds as one, each planned on its own (measured 2 % faster end to end than one launch with the mixed epilogue)
inline bool gemm_qkv_splits(int M, int N, int vt_col0, int ldc, int ldvt, const GemmSwitches& sw) {
    const int nv = N - vt_col0;
    const bool small_grid = (long long)(M / 256) * (N / 256) < 128 && sw.small_v1;
    return sw.qkv_split && !small_grid && M % 256 == 0 && vt_col0 % 256 == 0 && nv % 256 == 0 && nv > 0 && ldc % 8 == 0 && ldvt % 8 == 0;
}
