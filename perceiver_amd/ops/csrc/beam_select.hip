// Beam search on the captured-graph decode path: the per-group beam top-k
// (beam_select) and the in-place permutation of the generated KV-cache rows
// (beam_reorder). Both read everything that can change between requests or
// steps (EOS id, fill id, cursors, cache lengths, start rows, the permutation)
// from device memory, so one captured graph serves every request.
//
// beam_select, one block per group of num_beams rows:
//   1. the group's old state (score, done, gen_len) is staged in LDS;
//   2. max and log-sum-exp of every live row: one wave per row (V <= 1024) or
//      the whole block per row, in both cases through a lane layout and a
//      reduction tree that do not depend on the row, so identical rows give
//      identical bits and two runs agree bit for bit;
//   3. candidate (i, v) is score_i + ((x_iv - max_i) - lse_i) in fp32, or for
//      a frozen row score_i + 0 at the fill token and score_i + (-1e9)
//      elsewhere. It is packed as (order key << 32) | ~(i V + v): a max over
//      the packed word orders by candidate descending, flat index ascending;
//   4. one pass over the candidates in which every thread keeps its own eight
//      largest, sorted, in registers, then num_beams rounds of "largest packed
//      word strictly below the previous winner" over those: exact, sort-free;
//   5. lanes 0..num_beams-1 write the bookkeeping from the staged state.
// Two tiers (docs/kernels.md): num_beams * V <= 4096 runs 256 threads, larger
// groups 1024 so that four waves per SIMD hide the element-wise loads.
//
// beam_reorder, one launch for all cache buffers: the thread that owns one
// (group, row, 16-B unit) reads all num_beams source units before it writes
// any, so the permutation is in place and nothing crosses threads.
#include <ATen/cuda/CUDAContext.h>
#include "common.h"
#include "select_common.h"

namespace {

constexpr int BS_THREADS = 256;       // groups of up to BS_SMALL_GROUP candidates
constexpr int BS_BIG_THREADS = 1024;  // larger groups: four waves per SIMD hide the loads
constexpr int BS_SMALL_GROUP = 4096;
constexpr int BS_WAVE_ROW_MAXV = 1024;
constexpr int BS_MIN_BEAMS = 2;
constexpr int BS_MAX_BEAMS = 8;
constexpr int BS_MAXV = 32768;  // decode_select_applicable's range

struct BeamArgs {
    const void* logits;  // (G * nb, V), last dim contiguous
    long row_stride;     // elements
    int G, nb, V;
    float* score;               // (G * nb) running scores, in and out
    unsigned char* done;        // (G * nb) bool, in and out
    int* gen_len;               // (G * nb), in and out
    long long* tok;             // (G * nb) out: the token the next step embeds
    int* src;                   // (G * nb) out: source beam inside the group
    unsigned char* all_done;    // (G) out: every beam of the group is done
    const long long* eos_fill;  // (2): eos id (< 0: none), fill id
    const long long* step;      // (1) record cursor, or null for 0
    int rec_offset;             // the record row is *step + rec_offset
    int rec_rows;
    long long* rec_tok;           // (rec_rows, G * nb) or null
    int* rec_parent;              // (rec_rows, G * nb)
    unsigned char* rec_all_done;  // (rec_rows, G)
};

template <int THREADS>
struct GroupState {
    float score[BS_MAX_BEAMS], xmax[BS_MAX_BEAMS], lse[BS_MAX_BEAMS];
    int gen_len[BS_MAX_BEAMS];
    int done[BS_MAX_BEAMS];
    unsigned long long red[THREADS / WAVE];
    float redf[THREADS / WAVE];
    unsigned long long win[BS_MAX_BEAMS];
};

template <typename T, typename State>
DEVINL unsigned long long candidate(const State& st, const T* rows, long row_stride, int V,
                                    int fill, int i, int v) {
    float c;
    if (st.done[i]) {
        c = st.score[i] + (v == fill ? 0.f : -1e9f);
    } else {
        const float x = load_logit(rows + (long)i * row_stride, v);
        c = st.score[i] + ((x - st.xmax[i]) - st.lse[i]);
    }
    return pack_best(order_key(c), i * V + v);
}

// max / sum over the block, combined in wave order; every thread gets the result
template <int THREADS>
DEVINL unsigned long long block_max_u64(GroupState<THREADS>& st, unsigned long long v) {
    v = wave_max_u64(v);
    __syncthreads();  // the previous result has been read by everyone
    if ((threadIdx.x & (WAVE - 1)) == 0) st.red[threadIdx.x / WAVE] = v;
    __syncthreads();
    unsigned long long r = st.red[0];
#pragma unroll
    for (int w = 1; w < THREADS / WAVE; ++w) r = st.red[w] > r ? st.red[w] : r;
    return r;
}
template <int THREADS>
DEVINL float block_sum_f(GroupState<THREADS>& st, float v) {
    v = wave_sum_f(v);
    __syncthreads();
    if ((threadIdx.x & (WAVE - 1)) == 0) st.redf[threadIdx.x / WAVE] = v;
    __syncthreads();
    float r = st.redf[0];
#pragma unroll
    for (int w = 1; w < THREADS / WAVE; ++w) r += st.redf[w];
    return r;
}

template <typename T, int THREADS>
__global__ __launch_bounds__(THREADS) void beam_select_kernel(BeamArgs a) {
    __shared__ GroupState<THREADS> st;
    const int g = blockIdx.x, tid = threadIdx.x, lane = tid & (WAVE - 1);
    const int nb = a.nb, V = a.V;
    const long row0 = (long)g * nb;
    const T* rows = reinterpret_cast<const T*>(a.logits) + row0 * a.row_stride;

    // all of the group's old state is read before any of it is written
    if (tid < nb) {
        st.score[tid] = a.score[row0 + tid];
        st.done[tid] = a.done[row0 + tid] != 0;
        st.gen_len[tid] = a.gen_len[row0 + tid];
        st.xmax[tid] = 0.f;
        st.lse[tid] = 0.f;
    }
    __syncthreads();
    // max and log-sum-exp of every live row, through a tree that does not
    // depend on the row: a wave per row for short rows, the block per row above
    if (V <= BS_WAVE_ROW_MAXV) {
        for (int i = tid / WAVE; i < nb; i += THREADS / WAVE) {
            if (st.done[i]) continue;  // wave-uniform
            const T* row = rows + (long)i * a.row_stride;
            unsigned int km = 0;
            for (int v = lane; v < V; v += WAVE) {
                const unsigned int k = order_key(load_logit(row, v));
                km = k > km ? k : km;
            }
            const float xmax = key_value(wave_max_u(km));
            float s = 0.f;
            for (int v = lane; v < V; v += WAVE) s += expf(load_logit(row, v) - xmax);
            s = wave_sum_f(s);
            if (lane == 0) {
                st.xmax[i] = xmax;
                st.lse[i] = logf(s);
            }
        }
    } else {
        for (int i = 0; i < nb; ++i) {
            if (st.done[i]) continue;  // block-uniform
            const T* row = rows + (long)i * a.row_stride;
            unsigned int km = 0;
#pragma unroll 4
            for (int v = tid; v < V; v += THREADS) {
                const unsigned int k = order_key(load_logit(row, v));
                km = k > km ? k : km;
            }
            const float xmax = key_value((unsigned int)(block_max_u64(st, km)));
            float s = 0.f;
#pragma unroll 4
            for (int v = tid; v < V; v += THREADS) s += expf(load_logit(row, v) - xmax);
            s = block_sum_f(st, s);
            if (tid == 0) {
                st.xmax[i] = xmax;
                st.lse[i] = logf(s);
            }
        }
    }
    __syncthreads();

    // one pass over the group's candidates: every thread keeps the largest
    // BS_MAX_BEAMS of its own, sorted, in registers (compile-time indices only).
    // The group's num_beams best are among the threads' num_beams best.
    const int fill = (int)a.eos_fill[1];
    const int total = nb * V;
    unsigned long long top[BS_MAX_BEAMS] = {};
    for (int i = 0; i < nb; ++i) {
#pragma unroll 4
        for (int v = tid; v < V; v += THREADS) {
            const unsigned long long q = candidate(st, rows, a.row_stride, V, fill, i, v);
            if (q > top[BS_MAX_BEAMS - 1]) {
                top[BS_MAX_BEAMS - 1] = q;
#pragma unroll
                for (int k = BS_MAX_BEAMS - 1; k > 0; --k) {
                    const unsigned long long hi = top[k] > top[k - 1] ? top[k] : top[k - 1];
                    const unsigned long long lo = top[k] > top[k - 1] ? top[k - 1] : top[k];
                    top[k - 1] = hi;
                    top[k] = lo;
                }
            }
        }
    }
    // num_beams rounds of "largest packed word strictly below the previous winner"
    unsigned long long prev = 0ull;
    for (int j = 0; j < nb; ++j) {
        unsigned long long b = 0ull;
#pragma unroll
        for (int k = 0; k < BS_MAX_BEAMS; ++k) {
            const unsigned long long q = top[k];
            b = ((j == 0 || q < prev) && q > b) ? q : b;
        }
        prev = block_max_u64(st, b);
        if (tid == 0) st.win[j] = prev;
    }
    __syncthreads();
    if (tid >= WAVE) return;

    bool d = true;  // lanes past nb do not hold the group back
    if (tid < nb) {
        const unsigned long long w = st.win[tid];
        int f = best_index(w);
        f = f < 0 ? 0 : (f >= total ? total - 1 : f);
        const int s = f / V;
        const long long t = f - s * V;
        const bool was = st.done[s] != 0;
        d = was || t == a.eos_fill[0];
        const long row = row0 + tid;
        a.score[row] = key_value((unsigned int)(w >> 32));
        a.done[row] = d ? 1 : 0;
        a.gen_len[row] = st.gen_len[s] + (was ? 0 : 1);
        a.tok[row] = t;
        a.src[row] = s;
        const long long cur = (a.step ? *a.step : 0ll) + a.rec_offset;
        if (a.rec_tok && cur >= 0 && cur < a.rec_rows) {
            a.rec_tok[cur * ((long)a.G * nb) + row] = t;
            a.rec_parent[cur * ((long)a.G * nb) + row] = s;
        }
    }
    const bool all = __all(d);
    if (tid == 0) {
        a.all_done[g] = all ? 1 : 0;
        const long long cur = (a.step ? *a.step : 0ll) + a.rec_offset;
        if (a.rec_all_done && cur >= 0 && cur < a.rec_rows) a.rec_all_done[cur * a.G + g] = all ? 1 : 0;
    }
}

template <typename T>
void launch_beam_select(const BeamArgs& a) {
    auto stream = at::cuda::getCurrentCUDAStream();
    if (a.nb * a.V <= BS_SMALL_GROUP)
        hipLaunchKernelGGL((beam_select_kernel<T, BS_THREADS>), dim3(a.G), dim3(BS_THREADS), 0,
                           stream, a);
    else
        hipLaunchKernelGGL((beam_select_kernel<T, BS_BIG_THREADS>), dim3(a.G),
                           dim3(BS_BIG_THREADS), 0, stream, a);
    HIP_CHECK_LAST();
}

template <typename P>
P* state_ptr(const torch::Tensor& t, torch::ScalarType st, long n, const torch::Tensor& like,
             const char* name) {
    TORCH_CHECK(t.device() == like.device() && t.scalar_type() == st && t.numel() == n &&
                    t.is_contiguous(),
                "beam_select: ", name, " must be a contiguous tensor of ", n,
                " element(s) of the right dtype on the logits' device");
    return reinterpret_cast<P*>(t.data_ptr());
}

// ---- beam_reorder ----

constexpr int BR_THREADS = 256;
constexpr int BR_ROW_BLOCKS = 32;
constexpr int BR_FIELDS = 6;  // base pointer, capacity, units per row, unit bytes, row0, counter index

typedef __attribute__((ext_vector_type(4))) unsigned int uint4v;

template <int NB, typename U>
DEVINL void reorder_rows(U* base, long cap, long upr, long row0, long len, int g,
                         const int (&s)[NB]) {
    for (long r = row0 + blockIdx.x; r <= len; r += gridDim.x) {
        for (long u = threadIdx.x; u < upr; u += BR_THREADS) {
            U v[NB];
#pragma unroll
            for (int i = 0; i < NB; ++i) v[i] = base[(((long)g * NB + i) * cap + r) * upr + u];
#pragma unroll
            for (int j = 0; j < NB; ++j) {
                if (s[j] == j) continue;  // block-uniform
                U val = v[0];
#pragma unroll
                for (int i = 1; i < NB; ++i) val = s[j] == i ? v[i] : val;
                base[(((long)g * NB + j) * cap + r) * upr + u] = val;
            }
        }
    }
}

// grid (row blocks, buffers, groups): static, since it is captured; a block
// strides over the rows [row0, len] of its (buffer, group) and leaves at once
// when the group's permutation is the identity
template <int NB>
__global__ __launch_bounds__(BR_THREADS) void beam_reorder_kernel(
    const long long* __restrict__ table, const long long* __restrict__ counters, int ncounters,
    const int* __restrict__ src) {
    const int g = blockIdx.z;
    int s[NB];
    bool identity = true;
#pragma unroll
    for (int j = 0; j < NB; ++j) {
        const int v = src[g * NB + j];
        s[j] = v < 0 ? 0 : (v >= NB ? NB - 1 : v);
        identity = identity && s[j] == j;
    }
    if (identity) return;
    const long long* d = table + (long)blockIdx.y * BR_FIELDS;
    const long cap = d[1], upr = d[2];
    const long row0 = d[4] < 0 ? 0 : d[4];
    const long ci = d[5] < 0 ? 0 : (d[5] >= ncounters ? ncounters - 1 : d[5]);
    long len = counters[ci];
    len = len >= cap ? cap - 1 : len;
    if (d[3] == 16) reorder_rows<NB>(reinterpret_cast<uint4v*>(d[0]), cap, upr, row0, len, g, s);
    else reorder_rows<NB>(reinterpret_cast<unsigned short*>(d[0]), cap, upr, row0, len, g, s);
}

template <int NB>
void launch_beam_reorder(const long long* table, int nbuf, const long long* counters,
                         int ncounters, const int* src, int groups) {
    hipLaunchKernelGGL((beam_reorder_kernel<NB>), dim3(BR_ROW_BLOCKS, nbuf, groups),
                       dim3(BR_THREADS), 0, at::cuda::getCurrentCUDAStream(), table, counters,
                       ncounters, src);
}

}  // namespace

bool beam_select_applicable(long V, long num_beams) {
    return V >= 1 && V <= BS_MAXV && num_beams >= BS_MIN_BEAMS && num_beams <= BS_MAX_BEAMS;
}

// One beam-search step for G groups of num_beams rows: scores, done, gen_len
// are updated in place; tok, src and all_done are written. With the record
// buffers the step's (token, parent, all-done) land in row *step + rec_offset.
void beam_select(torch::Tensor logits, torch::Tensor score, torch::Tensor done,
                 torch::Tensor gen_len, torch::Tensor tok, torch::Tensor src,
                 torch::Tensor all_done, torch::Tensor eos_fill, int64_t num_beams,
                 c10::optional<torch::Tensor> step, int64_t rec_offset,
                 c10::optional<torch::Tensor> rec_tok, c10::optional<torch::Tensor> rec_parent,
                 c10::optional<torch::Tensor> rec_all_done) {
    TORCH_CHECK(logits.is_cuda() && logits.dim() == 2, "beam_select: logits must be (B, V) on the GPU");
    TORCH_CHECK(logits.scalar_type() == torch::kBFloat16 || logits.scalar_type() == torch::kFloat32,
                "beam_select: logits must be bf16 or fp32");
    const long B = logits.size(0), V = logits.size(1);
    TORCH_CHECK(beam_select_applicable(V, num_beams),
                "beam_select: V or num_beams out of range (beam_select_applicable)");
    TORCH_CHECK(B > 0 && B < (1L << 24) && B % num_beams == 0,
                "beam_select: the batch must be a multiple of num_beams");
    TORCH_CHECK(logits.stride(1) == 1 || V == 1, "beam_select: the vocabulary dim must be contiguous");
    BeamArgs a = {};
    a.logits = logits.data_ptr();
    a.row_stride = logits.stride(0);
    a.nb = (int)num_beams;
    a.G = (int)(B / num_beams);
    a.V = (int)V;
    a.score = state_ptr<float>(score, torch::kFloat32, B, logits, "score");
    a.done = state_ptr<unsigned char>(done, torch::kBool, B, logits, "done");
    a.gen_len = state_ptr<int>(gen_len, torch::kInt32, B, logits, "gen_len");
    a.tok = state_ptr<long long>(tok, torch::kInt64, B, logits, "tok");
    a.src = state_ptr<int>(src, torch::kInt32, B, logits, "src");
    a.all_done = state_ptr<unsigned char>(all_done, torch::kBool, a.G, logits, "all_done");
    a.eos_fill = state_ptr<const long long>(eos_fill, torch::kInt64, 2, logits, "eos_fill");
    if (has_tensor(step)) a.step = state_ptr<const long long>(*step, torch::kInt64, 1, logits, "step");
    a.rec_offset = (int)rec_offset;
    if (has_tensor(rec_tok)) {
        TORCH_CHECK(has_tensor(rec_parent) && has_tensor(rec_all_done) && rec_tok->dim() == 2,
                    "beam_select: the record needs rec_tok (rows, B), rec_parent and rec_all_done");
        const long rows = rec_tok->size(0);
        a.rec_rows = (int)rows;
        a.rec_tok = state_ptr<long long>(*rec_tok, torch::kInt64, rows * B, logits, "rec_tok");
        a.rec_parent = state_ptr<int>(*rec_parent, torch::kInt32, rows * B, logits, "rec_parent");
        a.rec_all_done =
            state_ptr<unsigned char>(*rec_all_done, torch::kBool, rows * a.G, logits, "rec_all_done");
    }
    if (logits.scalar_type() == torch::kFloat32) launch_beam_select<float>(a);
    else launch_beam_select<unsigned short>(a);
}

// In-place permutation of rows [row0, len] of every buffer of the descriptor
// table by the per-group source beams in src. table is (nbuf, 6) int64 on the
// device, built by ops/beam.py::reorder_table, which checks the buffers.
void beam_reorder(torch::Tensor table, torch::Tensor counters, torch::Tensor src,
                  int64_t num_beams) {
    TORCH_CHECK(table.is_cuda() && table.scalar_type() == torch::kInt64 && table.dim() == 2 &&
                    table.size(1) == BR_FIELDS && table.is_contiguous() && table.size(0) >= 1 &&
                    table.size(0) < 65536,
                "beam_reorder: table must be a contiguous (nbuf, 6) int64 tensor on the GPU");
    TORCH_CHECK(counters.device() == table.device() && counters.scalar_type() == torch::kInt64 &&
                    counters.is_contiguous() && counters.numel() >= 1,
                "beam_reorder: counters must be a contiguous int64 tensor on the table's device");
    TORCH_CHECK(num_beams >= BS_MIN_BEAMS && num_beams <= BS_MAX_BEAMS,
                "beam_reorder: num_beams out of range");
    TORCH_CHECK(src.device() == table.device() && src.scalar_type() == torch::kInt32 &&
                    src.is_contiguous() && src.numel() >= num_beams &&
                    src.numel() % num_beams == 0 && src.numel() / num_beams < 65536,
                "beam_reorder: src must be a contiguous (groups * num_beams) int32 tensor");
    const long long* t = reinterpret_cast<const long long*>(table.data_ptr<int64_t>());
    const long long* c = reinterpret_cast<const long long*>(counters.data_ptr<int64_t>());
    const int* s = src.data_ptr<int>();
    const int nbuf = (int)table.size(0), nc = (int)counters.numel();
    const int groups = (int)(src.numel() / num_beams);
    switch (num_beams) {
        case 2: launch_beam_reorder<2>(t, nbuf, c, nc, s, groups); break;
        case 3: launch_beam_reorder<3>(t, nbuf, c, nc, s, groups); break;
        case 4: launch_beam_reorder<4>(t, nbuf, c, nc, s, groups); break;
        case 5: launch_beam_reorder<5>(t, nbuf, c, nc, s, groups); break;
        case 6: launch_beam_reorder<6>(t, nbuf, c, nc, s, groups); break;
        case 7: launch_beam_reorder<7>(t, nbuf, c, nc, s, groups); break;
        default: launch_beam_reorder<8>(t, nbuf, c, nc, s, groups); break;
    }
    HIP_CHECK_LAST();
}
