// Order-preserving keys, packed (key, index) maxima, element-wise logit loads
// and the wave reductions shared by the selection kernels (decode_select.hip,
// beam_select.hip).
#pragma once

#include "common.h"

// order-preserving image of an fp32 value: a < b <=> key(a) < key(b). NaN (of
// either sign) maps to the top so it compares as largest, as torch's argmax
// has it; -0 ties +0. No real value maps to 0, which marks an absent slot.
DEVINL unsigned int order_key(float x) {
    if (x != x) return 0xFFFFFFFFu;
    unsigned int u = (x == 0.f) ? 0u : __float_as_uint(x);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

DEVINL float key_value(unsigned int k) {
    return __uint_as_float((k & 0x80000000u) ? (k & 0x7FFFFFFFu) : ~k);
}

// (key, lowest index wins) as one 64-bit word for a max-reduction
DEVINL unsigned long long pack_best(unsigned int key, int idx) {
    return ((unsigned long long)key << 32) | (unsigned int)(0xFFFFFFFFu - (unsigned int)idx);
}
DEVINL int best_index(unsigned long long p) { return (int)(0xFFFFFFFFu - (unsigned int)p); }

DEVINL float load_logit(const float* p, long i) { return p[i]; }
DEVINL float load_logit(const unsigned short* p, long i) { return bf2f(p[i]); }

// ---- wave reductions: xor butterflies, every lane ends with the same value ----
DEVINL float wave_sum_f(float x) {
#pragma unroll
    for (int m = 1; m < WAVE; m <<= 1) x += __shfl_xor(x, m, WAVE);
    return x;
}
DEVINL unsigned int wave_sum_u(unsigned int x) {
#pragma unroll
    for (int m = 1; m < WAVE; m <<= 1) x += __shfl_xor(x, m, WAVE);
    return x;
}
DEVINL unsigned int wave_max_u(unsigned int x) {
#pragma unroll
    for (int m = 1; m < WAVE; m <<= 1) {
        unsigned int o = __shfl_xor(x, m, WAVE);
        x = o > x ? o : x;
    }
    return x;
}
DEVINL unsigned long long wave_max_u64(unsigned long long x) {
#pragma unroll
    for (int m = 1; m < WAVE; m <<= 1) {
        unsigned int lo = __shfl_xor((unsigned int)x, m, WAVE);
        unsigned int hi = __shfl_xor((unsigned int)(x >> 32), m, WAVE);
        unsigned long long o = ((unsigned long long)hi << 32) | lo;
        x = o > x ? o : x;
    }
    return x;
}
