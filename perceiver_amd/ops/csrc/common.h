// Shared helpers for the perceiver_amd CDNA4 (gfx950) kernels.
#pragma once

#include <torch/extension.h>
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdlib>

#define DEVINL __device__ __forceinline__

// wave64 is the CDNA scheduling quantum; hard-coded per the CDNA4 guide.
constexpr int WAVE = 64;

// vector types for wide loads (guideline 13: always vectorize bf16)
typedef __attribute__((ext_vector_type(4))) short short4v;
typedef __attribute__((ext_vector_type(8))) short short8v;
typedef __attribute__((ext_vector_type(4))) float float4v;
typedef __attribute__((ext_vector_type(2))) float float2v;
typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;
typedef __attribute__((ext_vector_type(4))) __bf16 bf16x4;

// bf16 <-> f32 on raw bits (round-to-nearest-even); avoids the hip_bf16 C++ API.
DEVINL float bf2f(unsigned short b) {
    unsigned int u = ((unsigned int)b) << 16;
    float f;
    __builtin_memcpy(&f, &u, 4);
    return f;
}

typedef __attribute__((ext_vector_type(2))) __bf16 bf16x2_t;

// packed pair convert: ONE v_cvt_pk_bf16_f32 for two floats (the scalar
// form needs 2 converts + shift + or); used by the P/dS image packing
DEVINL unsigned int f2bf2(float a, float b) {
    float2v f = {a, b};
    bf16x2_t p = __builtin_convertvector(f, bf16x2_t);
    unsigned int u;
    __builtin_memcpy(&u, &p, 4);
    return u;
}

typedef __attribute__((ext_vector_type(2))) unsigned int uint2v;

// four floats -> one 8-B store (two v_cvt_pk + one ds_write_b64): the two
// 4-B stores per lane at 32-B stride were a 2-way LDS bank conflict on the
// packed P/dS images (PMC: 10-12% of wave cycles)
DEVINL uint2v f2bf4(float a, float b, float c, float d) {
    return uint2v{f2bf2(a, b), f2bf2(c, d)};
}

DEVINL unsigned short f2bf(float f) {
    // native single-instruction convert (v_cvt_pk_bf16_f32, RTNE on gfx950);
    // the manual bit-math round used to cost 3-4 VALU ops per convert and
    // f2bf sits in every epilogue and the softmax P-packing hot paths
    __bf16 b = (__bf16)f;
    unsigned short u;
    __builtin_memcpy(&u, &b, 2);
    return u;
}

// counter-based RNG for attention dropout: the same (seed, bh, i, j) always
// yields the same draw, so the backward regenerates the forward's mask
// exactly without storing it. 32-bit combine + murmur3-style finalizer: the
// original splitmix64 chain lowered to ~3x the VALU ops, and the hash runs
// once per attention element — it was a measurable share of the backward
// kernels' 21:1 VALU:MFMA instruction ratio (profiles/ PMC).
// How the attention kernels split one hash into per-row 16-bit draws is
// written once in attn_common.h.
DEVINL unsigned int rng_hash(unsigned long long seed, int bh, int i, int j) {
    unsigned int x = (unsigned int)seed + (unsigned int)(seed >> 32) * 0x9E3779B9u;
    x += (unsigned int)bh * 0x85EBCA6Bu + (unsigned int)i * 0xC2B2AE35u +
         (unsigned int)j * 0x27D4EB2Fu;
    x ^= x >> 16;
    x *= 0x7FEB352Du;
    x ^= x >> 15;
    x *= 0x846CA68Bu;
    x ^= x >> 16;
    return x;
}

// erf via the Abramowitz-Stegun 7.1.26 rational approximation (|err| <=
// 1.5e-7 absolute — below bf16 output resolution, so GELU results match the
// exact-erf torch.nn.GELU after rounding). libm's float-exact erff costs
// several times more VALU and made the fused GELU kernels compute-bound.
DEVINL float erf_fast(float x) {
    const float ax = fabsf(x);
    const float t = __frcp_rn(1.0f + 0.3275911f * ax);
    float poly = 1.061405429f;
    poly = poly * t - 1.453152027f;
    poly = poly * t + 1.421413741f;
    poly = poly * t - 0.284496736f;
    poly = poly * t + 0.254829592f;
    float e = 1.0f - poly * t * __expf(-ax * ax);
    return copysignf(e, x);
}

// GELU matching torch.nn.GELU default (erf form) to bf16 output precision
DEVINL float gelu_f(float x) { return 0.5f * x * (1.0f + erf_fast(x * 0.70710678118654752440f)); }

DEVINL float gelu_grad_f(float x) {
    const float kInvSqrt2 = 0.70710678118654752440f;
    const float kInvSqrt2Pi = 0.39894228040143267794f;
    float cdf = 0.5f * (1.0f + erf_fast(x * kInvSqrt2));
    float pdf = kInvSqrt2Pi * __expf(-0.5f * x * x);
    return cdf + x * pdf;
}

// 8 channels c0..c0+7 of a global row of d channels, zero past d: one 16-B
// load for a full granule, element-wise on the ragged last one
DEVINL short8v load_granule_guarded(const unsigned short* __restrict__ row, int c0, int d) {
    short8v val = {};
    if (c0 + 8 <= d) {
        val = *reinterpret_cast<const short8v*>(row + c0);
    } else {
#pragma unroll
        for (int e = 0; e < 8; ++e) val[e] = (c0 + e < d) ? (short)row[c0 + e] : (short)0;
    }
    return val;
}

// XCD-aware bijective block order for a 1-D grid of nwg workgroups: hardware
// deals consecutive block ids round-robin over the 8 XCDs, so this hands each
// XCD a contiguous run of logical ids and neighbouring tiles (which share
// operand rows) meet in one L2.
DEVINL int xcd_block_order(int bid, int nwg) {
    int q = nwg / 8, r = nwg % 8;
    int xcd = bid % 8, idx = bid / 8;
    return (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + idx;
}

// ---- host side ----

// raw bf16 bits of a tensor's storage, as the kernels take them
inline unsigned short* bf16_ptr(const torch::Tensor& t) {
    return reinterpret_cast<unsigned short*>(t.data_ptr());
}

inline bool has_tensor(const c10::optional<torch::Tensor>& t) {
    return t.has_value() && t->defined();
}

// null when the optional tensor (a bias, usually) is absent
inline const unsigned short* opt_bf16_ptr(const c10::optional<torch::Tensor>& t) {
    return has_tensor(t) ? bf16_ptr(*t) : nullptr;
}

// integer tuning knob from the environment; callers cache it in a static
inline long env_int(const char* name, long dflt) {
    const char* e = getenv(name);
    return e ? atol(e) : dflt;
}

// grid of a grid-stride elementwise kernel: one thread per item up to cap blocks
inline long elementwise_blocks(long items, int threads, long cap) {
    return std::max<long>(1, std::min((items + threads - 1) / threads, cap));
}

// Dynamic-LDS requests above the 64 KiB default need a per-kernel opt-in
// (the CU has 160 KiB).
template <auto Kernel>
inline void allow_dynamic_lds(size_t smem) {
    if (smem <= 65536) return;
    static bool raised = [] {
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(Kernel),
                                  hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
        return true;
    }();
    (void)raised;
}

#define HIP_CHECK_LAST()                                                            \
    do {                                                                            \
        hipError_t e = hipGetLastError();                                           \
        if (e != hipSuccess) {                                                      \
            TORCH_CHECK(false, "HIP kernel launch failed: ", hipGetErrorString(e)); \
        }                                                                           \
    } while (0)
