// Support layer shared by the flash attention kernels (flash_fwd.hip,
// flash_fwd_pipe.hip, flash_bwd.hip): LDS tile images and their staging,
// hardware-transpose fragment reads, 16-lane reductions, the dropout draw
// mapping, and the host-side launch planning. Each piece is defined once here.
#pragma once

#include "common.h"

// ---- 16-lane row reductions (C-layout rows live in 16-lane groups) ----
DEVINL float warp16_max(float x) {
#pragma unroll
    for (int m = 1; m < 16; m <<= 1) x = fmaxf(x, __shfl_xor(x, m, 64));
    return x;
}

DEVINL float warp16_sum(float x) {
#pragma unroll
    for (int m = 1; m < 16; m <<= 1) x += __shfl_xor(x, m, 64);
    return x;
}

// ---- LDS tile images ----
// Row-major: rows ldst_bytes apart (callers add +16 B row padding so 16-lane
// groups read b128 fragments conflict-free).
// 16-column-subtiled (guide T10): channel-subtile s holds a (rows x 16)
// row-major bf16 block with 16-elem (32 B) rows, subtiles padded by 8 elems
// (16 B) so consecutive subtiles shift LDS banks. ds_read_b64_tr_b16's gather
// (lane l elem j reads base + (l&15) + j*16 + (l>>4)*64) turns two reads of
// this image into the 32x16 MFMA B-fragment — the operand is staged ROW-major
// (one 16-B write per granule, no 8-row write lockstep: that pattern measured
// ~11% of wave cycles in bank conflicts) yet consumed column-major.
enum : int { IMG_RM = 1, IMG_SUB16 = 2 };

constexpr int sub16_elems(int rows) { return rows * 16 + 8; }

// store one 8-channel granule (row, c0..c0+7) into the selected images
template <int ROWS_TILE, int IMG>
DEVINL void store_granule(short8v val, int row, int c0, char* lds_rm, int ldst_bytes,
                          char* lds16) {
    if (IMG & IMG_RM) *reinterpret_cast<short8v*>(lds_rm + row * ldst_bytes + c0 * 2) = val;
    if (IMG & IMG_SUB16)
        *reinterpret_cast<short8v*>(
            lds16 + ((c0 / 16) * sub16_elems(ROWS_TILE) + row * 16 + (c0 % 16)) * 2) = val;
}

// Fragment (rows row0..row0+31, cols 16*sub..) from a subtiled image.
// Per-lane addressing: each 16-lane group loads one 4x16 row-major tile
// linearly (lane supplies its own 8-B chunk at lo16*4 elems) and the
// instruction's fixed cross-lane exchange delivers column lo16 to the lane;
// group hi4 starts at row hi4*8, the second read covers rows +4.
template <int ROWS_TILE>
DEVINL bf16x8 read_frag_tr16(const char* lds, int sub, int row0, int hi4, int lo16) {
    const __bf16* base = reinterpret_cast<const __bf16*>(lds) +
                         sub * sub16_elems(ROWS_TILE) + (row0 + hi4 * 8) * 16 + lo16 * 4;
    auto p = (__attribute__((address_space(3))) bf16x4*)base;
    bf16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4bf16(p);
    bf16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4bf16(p + 16);  // +4 rows
    bf16x8 out;
#pragma unroll
    for (int e = 0; e < 4; ++e) { out[e] = lo[e]; out[e + 4] = hi[e]; }
    return out;
}

// Guarded staging: (ROWS_TILE x d) bf16 tile from global (row stride src_stride
// elems) into the images selected by IMG, zero-filling row >= rows_valid and
// col >= d up to d_pad. One global read per granule whatever the image count.
template <int ROWS_TILE, int IMG>
DEVINL void stage_tile(const unsigned short* __restrict__ src, long src_stride,
                       int rows_valid, int d, int d_pad,
                       char* lds_rm, int ldst_bytes, char* lds16, int tid) {
    const int gpr = d_pad / 8;
    const int total = ROWS_TILE * gpr;
    for (int g = tid; g < total; g += 256) {
        int row = g / gpr;
        int c0 = (g % gpr) * 8;
        // granules wholly past d (c0 >= d) only need the explicit test where a
        // subtiled image is written; on a row-major-only tile the element-wise
        // branch of the loader already yields zeros for them without loading
        short8v val = {};
        if (row < rows_valid && (!(IMG & IMG_SUB16) || c0 < d))
            val = load_granule_guarded(src + (long)row * src_stride, c0, d);
        store_granule<ROWS_TILE, IMG>(val, row, c0, lds_rm, ldst_bytes, lds16);
    }
}

// Guarded A-fragment row: lane holds A[i][k = hi4*8 + e] per 32-wide k-block
// of a row of dim channels (nblocks live blocks); invalid rows load zeros.
template <int NB>
DEVINL void load_afrag_row(short8v (&frag)[NB], const unsigned short* __restrict__ row,
                           bool valid, int nblocks, int dim, int hi4) {
#pragma unroll
    for (int kb = 0; kb < NB; ++kb) {
        short8v val = {};
        if (kb < nblocks && valid) val = load_granule_guarded(row, kb * 32 + hi4 * 8, dim);
        frag[kb] = val;
    }
}

// ---- T14 async-STAGE split ----
// issue: clamped-row unconditional vector loads into registers; the vmcnt
// waits land at the write call one compute phase later, hiding HBM latency
// under MFMA work. Valid only when the runtime dims match the template
// exactly (every granule full-width; callers pad odd dims to the template).
template <int ROWS_TILE, int DD, int NG>
DEVINL void issue_tile(short8v (&st)[NG], const unsigned short* __restrict__ src,
                       long sstride, int row_limit, int tid) {
    constexpr int GPR = DD / 8;
#pragma unroll
    for (int i = 0; i < NG; ++i) {
        int g = tid + i * 256;
        int row = g / GPR, c0 = (g % GPR) * 8;
        int rowc = row < row_limit ? row : row_limit - 1;
        st[i] = *reinterpret_cast<const short8v*>(src + (long)rowc * sstride + c0);
    }
}

// write half: spill staged registers into the images selected by IMG,
// zero-filling clamp-duplicated tail rows
template <int ROWS_TILE, int DD, int IMG, int NG>
DEVINL void write_tile(const short8v (&st)[NG], char* lds_rm, int ldst_bytes, char* lds16,
                       int rows_valid, int tid) {
    constexpr int GPR = DD / 8;
    const bool tail = rows_valid < ROWS_TILE;
#pragma unroll
    for (int i = 0; i < NG; ++i) {
        int g = tid + i * 256;
        // NG rounds up for tiles that don't divide into whole 2048-elem
        // sweeps (288/352-wide pad tiers); the surplus granules are no-ops
        if ((ROWS_TILE * DD) % 2048 != 0 && g >= (ROWS_TILE * DD) / 8) continue;
        int row = g / GPR, c0 = (g % GPR) * 8;
        short8v val = st[i];
        if (tail && row >= rows_valid) val = short8v{};
        store_granule<ROWS_TILE, IMG>(val, row, c0, lds_rm, ldst_bytes, lds16);
    }
}

// ---- dropout draw mapping ----
// One 32-bit rng_hash at (seed, bh, qi >> 1, j) carries TWO 16-bit draws: the
// low half belongs to the even q row of the pair, the high half to the odd
// one. Forward and backward must regenerate identical masks, so this is the
// only place the mapping is written. The q-major pairing halves the hash VALU
// in the kernels whose inner r-loop walks consecutive q rows (both forwards,
// dq): they take drop_pair_hash once per row pair and drop_half per row; dkv
// walks keys and takes single draws through drop16.
// Keep threshold is 16-bit: drop_p quantized to 1/65536.
DEVINL unsigned int drop_pair_hash(unsigned long long seed, int bh, int qi, int j) {
    return rng_hash(seed, bh, qi >> 1, j);
}

DEVINL unsigned int drop_half(unsigned int pair_hash, int qi) {
    return (qi & 1) ? (pair_hash >> 16) : (pair_hash & 0xffffu);
}

DEVINL unsigned int drop16(unsigned long long seed, int bh, int qi, int j) {
    return drop_half(drop_pair_hash(seed, bh, qi, j), qi);
}

// ---- host side ----

// Split of a len-long reduction axis over gridDim.z when the natural grid
// (blocks workgroups) underfills the chip: aim for ~2 blocks per CU (512
// workgroups on 256 CUs), at least 4 tiles per split, at most 32 splits.
struct SplitPlan {
    int nsplit;
    long chunk;  // axis elements per split (a multiple of tile when nsplit > 1)
};

inline SplitPlan plan_split(long blocks, long len, int tile) {
    SplitPlan p{1, len};
    if (blocks < 512 && len > 4 * tile) {
        int want = (int)(512 / blocks) + 1;
        int max_split = (int)((len + 4 * tile - 1) / (4 * tile));
        int n = std::min({want, max_split, 32});
        long tiles = (len + tile - 1) / tile;
        p.chunk = (tiles + n - 1) / n * tile;
        p.nsplit = (int)((len + p.chunk - 1) / p.chunk);
    }
    return p;
}

// Forward KV-split: the plan plus the fp32 partial buffers (one slab per
// split) that flash_merge_kernel combines; empty when nsplit == 1.
struct FwdSplit {
    SplitPlan plan;
    long rows;  // B*H*Nq
    long len;   // Lk, the split axis
    torch::Tensor o_part, lse_part;
    float* o_part_p = nullptr;
    float* lse_part_p = nullptr;
};

inline FwdSplit make_fwd_split(const torch::Tensor& q, long Lk, long Dv, int qblk, int kvblk) {
    const long B = q.size(0), H = q.size(1), Nq = q.size(2);
    FwdSplit s{plan_split((Nq + qblk - 1) / qblk * B * H, Lk, kvblk), B * H * Nq, Lk};
    if (s.plan.nsplit > 1) {
        auto f32 = q.options().dtype(torch::kFloat32);
        s.o_part = torch::empty({(long)s.plan.nsplit, s.rows, Dv}, f32);
        s.lse_part = torch::empty({(long)s.plan.nsplit, s.rows}, f32);
        s.o_part_p = s.o_part.data_ptr<float>();
        s.lse_part_p = s.lse_part.data_ptr<float>();
    }
    return s;
}

// Odd large head dims (the img/flow D=261 class) run as the 288 template with
// zero-padded channels. Forward and backward must agree on this.
inline bool pads_to_288(long D, long Dv) {
    return D > 160 && (D != 288 || Dv != 288) && D <= 288 && Dv <= 288;
}

// (B, H, N, last) view of freshly allocated merged-heads (B, N, H, last)
// memory, for a result shaped like t (B, H, N, *): the module's head-merge
// transpose+reshape after attention then costs nothing.
inline torch::Tensor empty_merged_heads(const torch::Tensor& t, long last) {
    return torch::empty({t.size(0), t.size(2), t.size(1), last}, t.options()).permute({0, 2, 1, 3});
}

inline const bool* pad_mask_ptr(const c10::optional<torch::Tensor>& pad_mask) {
    return has_tensor(pad_mask) ? pad_mask->data_ptr<bool>() : nullptr;
}

// ---- the deep-pipelined forward's entry points (flash_fwd_pipe.hip) ----
// Every pipe template has 128-row workgroups and 64-key tiles; flash_fwd()
// plans the KV split for it with these.
constexpr int FLASH_PIPE_QBLK = 128;

bool flash_fwd_pipe_applicable(long D, long Dv, long Nq);
// Caller guarantees flash_fwd_pipe_applicable() and merges the split partials
// (same contract as the v3 kernel).
void flash_fwd_pipe_launch(const torch::Tensor& q, const torch::Tensor& k,
                           const torch::Tensor& v, const bool* padp, bool causal,
                           float drop_p, unsigned long long drop_seed,
                           torch::Tensor& out, torch::Tensor& lse, const FwdSplit& split);
