// Shared helpers for libtt_hip.so (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include "../../include/tt_hip.h"

// ---- element type of the 16-bit encoder path ---------------------------------------------------------------------------
// gemm.hip, attention.hip, rowops.hip and encoder_api.hip are compiled TWICE: as they are (bf16 activations and weights,
// v_mfma_*_bf16) and with -DTT_F16=1 (IEEE fp16, v_mfma_*_f16: the same matrix rate, three more mantissa bits at every
// rounding point -- FlagEmbedding's own default for these models, `precision="fp16"` here).  The second set's external
// functions carry an _f16 suffix (f16_names.h); everything that is not element arithmetic -- tile shapes, LDS images,
// copy schedules, the wait counts -- is the same source.  Code that is bf16 by definition (the split-bf16 planes, the fp8
// path's quantiser inputs, the scan) keeps the explicit bf16 helper names below and is dead code in the second set.
#ifndef TT_F16
#define TT_F16 0
#endif
#if TT_F16
#include "f16_names.h"
#endif

// ---- diagnostic build -------------------------------------------------------------------------------------------------------
// Switches that compute WRONG results by design (ablations of the scan loop, rounding masks of the reference-precision
// forward, the GEMM traffic / stamp experiments) or re-read the environment on every forward exist only in the diagnostic
// library, `make DIAG=1` -> libtt_hip_diag.so (tools/ and tools/probes/ load that one: TT_LIB_NAME).  In the product library
// TT_DIAG_ENV_INT is its default: a stray environment variable cannot change a score, and the ablation instantiations are
// not compiled.  A/B switches whose two sides give the same (or equally valid) results stay, read once into a static.
#ifndef TT_DIAG
#define TT_DIAG 0
#endif
// Round 5: the A/B switches of measured-and-rejected variants (TT_GEMM_SN, TT_ATT_WAVES, TT_SCAN_GEMM_*, ...) are
// diagnostic-only too: the product library reads NO environment variable (tests/test_lib_abi.py greps its strings), every switch
// is its default as a compile-time constant, and the instantiations only a non-default value could reach are not linked.
#if TT_DIAG
#define TT_DIAG_ENV_INT(name, dflt) ([]() -> int { const char* e_ = getenv(name); return e_ && e_[0] ? (int)strtol(e_, nullptr, 0) : (dflt); }())
#define TT_DIAG_ENV_FLOAT(name, dflt) ([]() -> float { const char* e_ = getenv(name); return e_ && e_[0] ? (float)atof(e_) : (dflt); }())
#else
#define TT_DIAG_ENV_INT(name, dflt) (dflt)
#define TT_DIAG_ENV_FLOAT(name, dflt) (dflt)
#endif

typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;
typedef __attribute__((ext_vector_type(16))) float f32x16;
typedef __attribute__((ext_vector_type(4))) float f32x4;

#define TT_WAVE 64

// thread-local error text (tt_last_error)
void tt_set_error(const char* fmt, ...);

#define TT_CHECK_ARG(cond, ...)            \
    do {                                   \
        if (!(cond)) {                     \
            tt_set_error(__VA_ARGS__);     \
            return TT_E_INVALID;           \
        }                                  \
    } while (0)

#define TT_CHECK_HIP(expr)                                                              \
    do {                                                                                \
        hipError_t _e = (expr);                                                         \
        if (_e != hipSuccess) {                                                         \
            tt_set_error("%s failed: %s (%s:%d)", #expr, hipGetErrorString(_e), __FILE__, __LINE__); \
            return TT_E_HIP;                                                            \
        }                                                                               \
    } while (0)

#define TT_CHECK_LAUNCH()                                                               \
    do {                                                                                \
        hipError_t _e = hipGetLastError();                                              \
        if (_e != hipSuccess) {                                                         \
            tt_set_error("kernel launch failed: %s (%s:%d)", hipGetErrorString(_e), __FILE__, __LINE__); \
            return TT_E_HIP;                                                            \
        }                                                                               \
    } while (0)

int tt_cu_count_cached();

// hipFuncSetAttribute(MaxDynamicSharedMemorySize) applies PER DEVICE: the "done" flag of a launch site is a bit mask
// over device ordinals (thread-local: no locking), so a thread that moves from GPU 0 to GPU 1 (one process driving
// several devices) opts the kernel in on the second device too.  Devices >= 64 always set it.
#define TT_SET_MAX_LDS(kern, bytes)                                                                              \
    do {                                                                                                         \
        static thread_local unsigned long long _tt_attr_mask = 0ull;                                             \
        int _tt_dev = 0;                                                                                         \
        TT_CHECK_HIP(hipGetDevice(&_tt_dev));                                                                    \
        if (_tt_dev >= 64 || !((_tt_attr_mask >> _tt_dev) & 1ull)) {                                             \
            TT_CHECK_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(kern),                                \
                                             hipFuncAttributeMaxDynamicSharedMemorySize, (int)(bytes)));         \
            if (_tt_dev < 64) _tt_attr_mask |= 1ull << _tt_dev;                                                  \
        }                                                                                                        \
    } while (0)

static inline size_t tt_align_up(size_t x, size_t a) { return (x + a - 1) / a * a; }

// ---- device helpers ---------------------------------------------------------
__device__ __forceinline__ float bf16_bits_to_f32(uint16_t h) {
    return __uint_as_float(((uint32_t)h) << 16);
}

// round-to-nearest-even f32 -> bf16 bits (NaN stays NaN through the compiler cast)
__device__ __forceinline__ uint16_t f32_to_bf16_bits(float f) {
    __bf16 b = (__bf16)f;
    return __builtin_bit_cast(uint16_t, b);
}

// two f32 -> packed bf16 pair, one v_cvt_pk_bf16_f32 (RNE; written as two scalar casts hipcc emits two
// conversions plus shift / or per pair: 4x the instructions in every epilogue)
typedef __bf16 bf16x2_t __attribute__((ext_vector_type(2)));
__device__ __forceinline__ uint32_t pack_bf16x2(float lo, float hi) {
    const bf16x2_t v = __builtin_convertvector(f32x2{lo, hi}, bf16x2_t);
    return __builtin_bit_cast(uint32_t, v);
}

// sum over the 64 lanes of a wave (butterfly: every lane ends with the same bits)
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// LDS reads hidden from the compiler's LDS-DMA tracking (it would put s_waitcnt vmcnt(0) in front of every ds_read while the
// next tile's copies are in flight), and the matching counted wait that names every destination register (x3_path.hip,
// f16c_path.hip; attention.hip and gemm.hip keep their own forms)
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
template <int OFF>
__device__ __forceinline__ u32x4 lds_read128(uint32_t addr) {
    u32x4 r;
    asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(r) : "v"(addr), "n"(OFF));
    return r;
}
template <int N>
__device__ __forceinline__ void lds_wait8(u32x4& a, u32x4& b, u32x4& c, u32x4& d, u32x4& e, u32x4& f, u32x4& g, u32x4& h) {
    asm volatile("s_waitcnt lgkmcnt(%8)" : "+v"(a), "+v"(b), "+v"(c), "+v"(d), "+v"(e), "+v"(f), "+v"(g), "+v"(h) : "n"(N));
}
template <int N>
__device__ __forceinline__ void lds_wait4(u32x4& a, u32x4& b, u32x4& c, u32x4& d) {
    asm volatile("s_waitcnt lgkmcnt(%4)" : "+v"(a), "+v"(b), "+v"(c), "+v"(d) : "n"(N));
}

// the embedding kernels' row indices: token id, position and type clamped into their tables (type == NULL: type 0)
__device__ __forceinline__ void embed_rows_clamped(const int32_t* ids, const int32_t* pos, const int32_t* type, int row, int vocab,
                                                   int max_pos, int type_vocab, int& id, int& p, int& t) {
    id = ids[row]; p = pos[row]; t = type ? type[row] : 0;
    id = id < 0 ? 0 : (id >= vocab ? vocab - 1 : id);
    p = p < 0 ? 0 : (p >= max_pos ? max_pos - 1 : p);
    t = t < 0 ? 0 : (t >= type_vocab ? type_vocab - 1 : t);
}

// ---- the element helpers the twice-compiled files use (see TT_F16 above) ---------------------------------------------------
constexpr bool kF16 = TT_F16 != 0;
#if TT_F16
typedef __attribute__((ext_vector_type(8))) _Float16 ex8;            // one MFMA operand fragment (8 elements per lane)
typedef _Float16 f16x2_t __attribute__((ext_vector_type(2)));
// low / high 16 bits of a dword as an element
__device__ __forceinline__ float elo(uint32_t u) { return (float)__builtin_bit_cast(f16x2_t, u).x; }
__device__ __forceinline__ float ehi(uint32_t u) { return (float)__builtin_bit_cast(f16x2_t, u).y; }
__device__ __forceinline__ float ebits_to_f32(uint16_t h) { return (float)__builtin_bit_cast(_Float16, h); }
// round to nearest even; finite values beyond the format's range saturate at +-65504 instead of becoming infinite
#ifndef TT_F16_SAT
#define TT_F16_SAT 1
#endif
// (a NaN stays a NaN: v_med3_f32 alone turns it into -65504 -- tests/test_gemm_edges_gpu.py, test_epilogue_sweep)
__device__ __forceinline__ float e_sat(float f) {
    const float c = __builtin_amdgcn_fmed3f(f, -65504.0f, 65504.0f);
    return TT_F16_SAT ? (f != f ? f : c) : f;
}
__device__ __forceinline__ uint16_t f32_to_ebits(float f) { return __builtin_bit_cast(uint16_t, (_Float16)e_sat(f)); }
__device__ __forceinline__ uint32_t pack_e2(float lo, float hi) {
    return __builtin_bit_cast(uint32_t, __builtin_convertvector(f32x2{e_sat(lo), e_sat(hi)}, f16x2_t));
}
// values known to be in range (softmax probabilities): no clamp
__device__ __forceinline__ uint32_t pack_e2_inrange(float lo, float hi) {
    return __builtin_bit_cast(uint32_t, __builtin_convertvector(f32x2{lo, hi}, f16x2_t));
}
#define TT_MFMA_16x16x32(a, b, c) __builtin_amdgcn_mfma_f32_16x16x32_f16((a), (b), (c), 0, 0, 0)
#define TT_MFMA_32x32x16(a, b, c) __builtin_amdgcn_mfma_f32_32x32x16_f16((a), (b), (c), 0, 0, 0)
#else
typedef bf16x8 ex8;
__device__ __forceinline__ float elo(uint32_t u) { return __uint_as_float(u << 16); }
__device__ __forceinline__ float ehi(uint32_t u) { return __uint_as_float(u & 0xFFFF0000u); }
__device__ __forceinline__ float ebits_to_f32(uint16_t h) { return bf16_bits_to_f32(h); }
__device__ __forceinline__ uint16_t f32_to_ebits(float f) { return f32_to_bf16_bits(f); }
__device__ __forceinline__ uint32_t pack_e2(float lo, float hi) { return pack_bf16x2(lo, hi); }
__device__ __forceinline__ uint32_t pack_e2_inrange(float lo, float hi) { return pack_bf16x2(lo, hi); }
#define TT_MFMA_16x16x32(a, b, c) __builtin_amdgcn_mfma_f32_16x16x32_bf16((a), (b), (c), 0, 0, 0)
#define TT_MFMA_32x32x16(a, b, c) __builtin_amdgcn_mfma_f32_32x32x16_bf16((a), (b), (c), 0, 0, 0)
#endif

// ---- per-kernel device timing (tt_prof_enable / tt_prof_read) -----------------------------
enum { TT_K_SCAN_FILTER = 1, TT_K_SCAN_SAMPLE = 2, TT_K_SELECT = 3, TT_K_GEMM = 4, TT_K_ATTENTION = 5, TT_K_ROWOPS = 6,
       TT_K_SCAN_TAIL = 7 /* streaming kernel over the < 256 tail rows behind the tiled filter pass */ };
bool tt_prof_on();
void tt_prof_begin(int id, hipStream_t st);
void tt_prof_end(hipStream_t st);
struct TtProfScope {
    hipStream_t st;
    bool on;
    TtProfScope(int id, hipStream_t s) : st(s), on(tt_prof_on()) { if (on) tt_prof_begin(id, st); }
    ~TtProfScope() { if (on) tt_prof_end(st); }
};
