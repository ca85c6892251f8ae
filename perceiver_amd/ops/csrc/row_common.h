// Support layer shared by the row-wise and column-reduction kernels
// (layer_norm.hip, colsum.hip): one wave64 walks a row of C <= 2048 bf16
// channels in CHUNKS = ceil(C / 512) chunks, each lane owning one 8-channel
// (16-B) granule per chunk. The wave reduction, the granule visitor, the
// tiled partial slab and the host-side launch planning are written once here.
// Which kernels keep a written-out walk instead of the visitor, and why, is
// in docs/kernels.md.
#pragma once

#include <type_traits>
#include "common.h"

// ---- wave reduction ----
DEVINL float wave_sum(float x) {
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) x += __shfl_xor(x, m, 64);
    return x;
}

// ---- granule walk ----
constexpr int ROW_MAXC = 2048;  // 4 chunks of 512 channels

// first channel of the lane's granule in chunk i
DEVINL int granule_col(int lane, int i) { return lane * 8 + i * 512; }

// Visit the granule c0..c0+7 of N rows of C channels: body(e, v) runs once per
// in-range element e with v[n] = rows[n][c0 + e] as float. A whole granule is
// N 16-B loads, the ragged last one guarded element loads. The branch is taken
// ONCE per granule and the body inlined into both arms, e stays a compile-time
// index (a runtime bound would push the callers' register arrays to scratch).
// Do not fold the two arms into a zero-filling load plus per-element select:
// that form spilled the wide LN backward instantiations (docs/kernels.md).
template <int N, typename Body>
DEVINL void visit_granule(const unsigned short* const (&rows)[N], int c0, int C, Body&& body) {
    if (c0 + 8 <= C) {
        short8v raw[N];
#pragma unroll
        for (int n = 0; n < N; ++n) raw[n] = *reinterpret_cast<const short8v*>(rows[n] + c0);
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            float v[N];
#pragma unroll
            for (int n = 0; n < N; ++n) v[n] = bf2f((unsigned short)raw[n][e]);
            body(e, v);
        }
    } else if (c0 < C) {
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            if (c0 + e < C) {
                float v[N];
#pragma unroll
                for (int n = 0; n < N; ++n) v[n] = bf2f(rows[n][c0 + e]);
                body(e, v);
            }
        }
    }
}

// The matching store: row[c0 + e] = bf16(val(e)) for the in-range elements,
// one 16-B store for a whole granule.
template <typename Val>
DEVINL void store_granule_bf16(unsigned short* row, int c0, int C, Val&& val) {
    if (c0 + 8 <= C) {
        short8v o;
#pragma unroll
        for (int e = 0; e < 8; ++e) o[e] = (short)f2bf(val(e));
        *reinterpret_cast<short8v*>(row + c0) = o;
    } else if (c0 < C) {
#pragma unroll
        for (int e = 0; e < 8; ++e)
            if (c0 + e < C) row[c0 + e] = f2bf(val(e));
    }
}

// ---- tiled fp32 partial slab ----
// Column sums leave the reduction kernels as one fp32 partial row per
// producer (a wave in colsum, a block in the LN backward), tiled
// [c >> 6][part][c & 63] so the finalize kernel streams 256-B bursts (a
// row-major slab cost it 16-32x DRAM amplification reading 4-B columns at a
// 4*C stride).
constexpr int SLAB_SHIFT = 6;
constexpr int SLAB_LANES = 1 << SLAB_SHIFT;

DEVINL long slab_index(int c, long part, long nparts) {
    return ((long)(c >> SLAB_SHIFT) * nparts + part) * SLAB_LANES + (c & (SLAB_LANES - 1));
}

// ---- host side ----

inline long slab_groups(long C) { return (C + SLAB_LANES - 1) / SLAB_LANES; }

inline torch::Tensor empty_slab(const torch::Tensor& like, long C, long nparts) {
    return torch::empty({slab_groups(C) * nparts, (long)SLAB_LANES},
                        like.options().dtype(torch::kFloat32));
}

// out[c] = sum over parts of the slab, c < C; out is fp32 or bf16 (colsum.hip)
void colsum_reduce_partials(const torch::Tensor& partial, torch::Tensor& out, int nparts, int C);

// f(std::integral_constant<int, CHUNKS>{}) for CHUNKS = ceil(C / 512) in 1..4
template <typename F>
inline void dispatch_chunks(int C, F&& f) {
    switch ((C + 511) / 512) {
        case 1: f(std::integral_constant<int, 1>{}); break;
        case 2: f(std::integral_constant<int, 2>{}); break;
        case 3: f(std::integral_constant<int, 3>{}); break;
        default: f(std::integral_constant<int, 4>{}); break;
    }
}

// Block count of a grid-stride row reduction (measured: 512 best for <= 32k
// rows, 1024 for 64k+; more blocks shrink rows/wave until latency dominates),
// never more blocks than there are rows to give every wave one.
// PERCEIVER_RED_BLOCKS moves the cap for sweeps.
inline long reduction_blocks(long rows, int waves_per_block) {
    static const long cap = env_int("PERCEIVER_RED_BLOCKS", 1024);
    long nblocks = std::min(std::max(rows / 32, (long)256), cap);
    return std::min(nblocks, (rows + waves_per_block - 1) / waves_per_block);
}
