// Fused token selection for the decode step: greedy argmax or temperature /
// top-k / top-p sampling of one token per batch row from the last-position
// logits, plus the decode bookkeeping (output record, EOS fill, done mask,
// token round-trip) in the same launch. Every sampling parameter is read from
// device memory and is per row, so one captured graph serves every sampling
// configuration of its batch size.
//
// Order is decided on the order-preserving unsigned image ("key") of the raw
// fp32 logit, never on the temperature-scaled value, so dividing by T cannot
// create or break ties. The k-th largest key and the nucleus boundary are both
// found by a 32-pass bitwise bisection over that key (compare-and-count,
// compare-and-add) on a row that already sits in registers or LDS: no sort.
// Every reduction runs in a fixed order (sums of masked terms through one
// tree), so the bisection predicate is monotone and two runs agree bit for bit.
//
// Two tiers (docs/kernels.md):
//   V <= 1024          one wave64 per row, 4 rows per block, the row in
//                      registers (ITEMS = ceil(V / 64) in a 1/2/4/8/16 ladder)
//   1024 < V <= 32768  one 256-thread block per row, the fp32 row in dynamic LDS
//
// The draw is Gumbel-max over the kept set with the counter hash rng_hash keyed
// by (seed, row, draw index, token). Counters (step cursor, draw index) are
// only READ here; the caller advances them with one add_ over the tensor they
// are views of, so no block races another on a counter.
#include <ATen/cuda/CUDAContext.h>
#include <type_traits>
#include "common.h"
#include "select_common.h"

namespace {

constexpr int DS_WAVE_MAXV = 1024;
constexpr int DS_BLOCK_MAXV = 32768;
constexpr int DS_THREADS = 256;
constexpr int DS_WAVES = DS_THREADS / WAVE;

struct SelectArgs {
    const void* logits;  // (B, V), last dim contiguous
    long row_stride;     // elements
    int B, V;
    const int* do_sample;      // (B)
    const float* temperature;  // (B)
    const int* top_k;          // (B)
    const float* top_p;        // (B)
    const long long* seed;     // (1)
    const long long* draw;     // (1)
    long long* tok;            // (B): previous token in (when out_buf), new token out
    long long* out_buf;        // (B, out_cols) or null
    long out_stride;
    int out_cols;
    const long long* step;     // (1), cursor into out_buf
    unsigned char* done;       // (B) bool or null
    const long long* eos_fill; // (2): eos id (< 0: none), fill id
    unsigned char* mask;       // (B, V) bool: debug output of the kept set
};

// log-weight + Gumbel noise of token idx; the uniform keeps 23 hash bits so
// that u stays strictly inside (0, 1) in fp32
DEVINL unsigned int gumbel_key(float logw, unsigned long long seed, int row, int draw, int idx) {
    unsigned int h = rng_hash(seed, row, draw, idx);
    float u = ((float)(h >> 9) + 0.5f) * (1.0f / 8388608.0f);
    return order_key(logw - logf(-logf(u)));
}

// ---- tier 1: one wave per row, the row in registers ----
template <int ITEMS>
struct WaveRow {
    unsigned int key[ITEMS];  // 0 on slots past V
    float lw[ITEMS];          // raw logit, then (x - max) / T
    float w[ITEMS];           // exp(lw)
    int lane, V;

    template <typename T>
    DEVINL void load(const T* row, int V_, float*) {
        V = V_;
        lane = threadIdx.x & (WAVE - 1);
#pragma unroll
        for (int i = 0; i < ITEMS; ++i) {
            int idx = lane + i * WAVE;
            bool ok = idx < V;
            float x = ok ? load_logit(row, idx) : 0.f;
            key[i] = ok ? order_key(x) : 0u;
            lw[i] = x;
        }
    }
    DEVINL unsigned long long max_packed() const {
        unsigned long long b = 0;
#pragma unroll
        for (int i = 0; i < ITEMS; ++i) {
            unsigned long long p = key[i] ? pack_best(key[i], lane + i * WAVE) : 0ull;
            b = p > b ? p : b;
        }
        return wave_max_u64(b);
    }
    DEVINL void set_softmax(float xmax, float inv_t) {
#pragma unroll
        for (int i = 0; i < ITEMS; ++i) {
            lw[i] = (lw[i] - xmax) * inv_t;
            w[i] = key[i] ? __expf(lw[i]) : 0.f;
        }
    }
    DEVINL unsigned int count_ge(unsigned int t) const {
        unsigned int n = 0;
#pragma unroll
        for (int i = 0; i < ITEMS; ++i) n += (unsigned int)__popcll(__ballot(key[i] >= t));
        return n;
    }
    // mass of the top-k set (key >= tk) strictly above key t
    DEVINL float mass_gt(unsigned int t, unsigned int tk) const {
        float s = 0.f;
#pragma unroll
        for (int i = 0; i < ITEMS; ++i) s += (key[i] > t && key[i] >= tk) ? w[i] : 0.f;
        return wave_sum_f(s);
    }
    DEVINL unsigned long long gumbel_best(unsigned int tkeep, unsigned long long seed, int row,
                                          int draw) const {
        unsigned long long b = 0;
#pragma unroll
        for (int i = 0; i < ITEMS; ++i) {
            int idx = lane + i * WAVE;
            if (key[i] >= tkeep) {
                unsigned long long p = pack_best(gumbel_key(lw[i], seed, row, draw, idx), idx);
                b = p > b ? p : b;
            }
        }
        return wave_max_u64(b);
    }
    DEVINL void write_mask(unsigned char* m, unsigned int tkeep) const {
#pragma unroll
        for (int i = 0; i < ITEMS; ++i) {
            int idx = lane + i * WAVE;
            if (idx < V) m[idx] = key[i] >= tkeep ? 1 : 0;
        }
    }
    DEVINL bool leader() const { return lane == 0; }
};

// ---- tier 2: one block per row, the fp32 row in LDS ----
struct BlockRow {
    float* x;                  // V floats of LDS
    unsigned long long* red;   // DS_WAVES words of LDS behind the row
    int tid, V;
    float xmax, inv_t;

    template <typename T>
    DEVINL void load(const T* row, int V_, float* lds) {
        V = V_;
        tid = threadIdx.x;
        x = lds;
        red = reinterpret_cast<unsigned long long*>(lds + ((V + 3) & ~3));
        for (int idx = tid; idx < V; idx += DS_THREADS) x[idx] = load_logit(row, idx);
        __syncthreads();
    }
    // combine the per-wave results in wave order; every thread gets the result
    template <typename V64, typename Op>
    DEVINL V64 across_waves(V64 v, Op op) const {
        __syncthreads();  // the previous result has been read by everyone
        if ((tid & (WAVE - 1)) == 0) __builtin_memcpy(&red[tid / WAVE], &v, sizeof(V64));
        __syncthreads();
        V64 r;
        __builtin_memcpy(&r, &red[0], sizeof(V64));
#pragma unroll
        for (int wv = 1; wv < DS_WAVES; ++wv) {
            V64 o;
            __builtin_memcpy(&o, &red[wv], sizeof(V64));
            r = op(r, o);
        }
        return r;
    }
    DEVINL unsigned long long max_packed() const {
        unsigned long long b = 0;
        for (int idx = tid; idx < V; idx += DS_THREADS) {
            unsigned long long p = pack_best(order_key(x[idx]), idx);
            b = p > b ? p : b;
        }
        return across_waves(wave_max_u64(b), [](unsigned long long a, unsigned long long c) {
            return a > c ? a : c;
        });
    }
    DEVINL void set_softmax(float xmax_, float inv_t_) { xmax = xmax_; inv_t = inv_t_; }
    DEVINL unsigned int count_ge(unsigned int t) const {
        unsigned int n = 0;
        for (int idx = tid; idx < V; idx += DS_THREADS) n += order_key(x[idx]) >= t ? 1u : 0u;
        return across_waves(wave_sum_u(n), [](unsigned int a, unsigned int c) { return a + c; });
    }
    DEVINL float mass_gt(unsigned int t, unsigned int tk) const {
        float s = 0.f;
        for (int idx = tid; idx < V; idx += DS_THREADS) {
            float v = x[idx];
            unsigned int k = order_key(v);
            // the exp is recomputed per pass: a second 128 KiB row does not fit
            if (k > t && k >= tk) s += __expf((v - xmax) * inv_t);
        }
        return across_waves(wave_sum_f(s), [](float a, float c) { return a + c; });
    }
    DEVINL unsigned long long gumbel_best(unsigned int tkeep, unsigned long long seed, int row,
                                          int draw) const {
        unsigned long long b = 0;
        for (int idx = tid; idx < V; idx += DS_THREADS) {
            float v = x[idx];
            if (order_key(v) >= tkeep) {
                unsigned long long p =
                    pack_best(gumbel_key((v - xmax) * inv_t, seed, row, draw, idx), idx);
                b = p > b ? p : b;
            }
        }
        return across_waves(wave_max_u64(b), [](unsigned long long a, unsigned long long c) {
            return a > c ? a : c;
        });
    }
    DEVINL void write_mask(unsigned char* m, unsigned int tkeep) const {
        for (int idx = tid; idx < V; idx += DS_THREADS) m[idx] = order_key(x[idx]) >= tkeep ? 1 : 0;
    }
    DEVINL bool leader() const { return tid == 0; }
};

// Smallest key that is kept: max of the k-th largest key and the nucleus
// boundary. Both the sampler and the keep_mask debug entry go through this.
template <typename Row>
DEVINL unsigned int keep_threshold(const Row& r, int top_k, float top_p) {
    unsigned int tk = 1;
    if (top_k > 0 && top_k < r.V) {
        // largest t with count(key >= t) >= k is the k-th largest key; ties stay
        unsigned int t = 0;
        for (int b = 31; b >= 0; --b) {
            unsigned int c = t | (1u << b);
            if (r.count_ge(c) >= (unsigned int)top_k) t = c;
        }
        tk = t > 1u ? t : 1u;
    }
    unsigned int tp = 1;
    if (top_p > 0.f && top_p < 1.f) {
        // token kept iff mass strictly above it <= top_p * Z. mass_gt is
        // non-increasing in t and mass_gt(0) = Z > top_p * Z, so the largest t
        // with mass_gt(t) > bound exists; keys above it are kept.
        const float bound = top_p * r.mass_gt(0u, tk);
        unsigned int t = 0;
        for (int b = 31; b >= 0; --b) {
            unsigned int c = t | (1u << b);
            if (r.mass_gt(c, tk) > bound) t = c;
        }
        tp = t + 1u;  // mass_gt(0xFFFFFFFF) = 0 is never above the bound: no wrap
    }
    return tk > tp ? tk : tp;
}

template <bool MASK, typename Row>
DEVINL void select_row(Row& r, const SelectArgs& a, int row) {
    const unsigned long long best = r.max_packed();
    int tokn = best_index(best);
    const float xmax = key_value((unsigned int)(best >> 32));
    const float T = a.temperature[row];
    // a row whose maximum is NaN or infinite has no softmax: it falls back to
    // the arg-max, which is always a valid index
    const bool finite = (xmax - xmax) == 0.f;
    const bool sample = (MASK || a.do_sample[row] != 0) && T > 0.f && finite;
    unsigned int tkeep = (unsigned int)(best >> 32);
    if (sample) {
        r.set_softmax(xmax, 1.0f / T);
        tkeep = keep_threshold(r, a.top_k[row], a.top_p[row]);
    }
    if (MASK) {
        r.write_mask(a.mask + (long)row * a.V, tkeep);
        return;
    }
    if (sample) {
        const unsigned long long g =
            r.gumbel_best(tkeep, (unsigned long long)*a.seed, row, (int)*a.draw);
        if (g != 0ull) tokn = best_index(g);
    }
    if (!r.leader()) return;
    tokn = tokn < 0 ? 0 : (tokn >= a.V ? a.V - 1 : tokn);
    long long t = tokn;
    if (a.out_buf) {
        const long long s = *a.step;
        if (s >= 0 && s < a.out_cols) a.out_buf[(long)row * a.out_stride + s] = a.tok[row];
    }
    if (a.done) {
        bool d = a.done[row] != 0;
        if (d) t = a.eos_fill[1];
        d = d || t == a.eos_fill[0];
        a.done[row] = d ? 1 : 0;
    }
    a.tok[row] = t;
}

template <typename T, int ITEMS, bool MASK>
__global__ __launch_bounds__(DS_THREADS) void decode_select_wave_kernel(SelectArgs a) {
    const int row = blockIdx.x * DS_WAVES + threadIdx.x / WAVE;
    if (row >= a.B) return;  // whole waves leave; this tier has no block barrier
    WaveRow<ITEMS> r;
    r.load(reinterpret_cast<const T*>(a.logits) + (long)row * a.row_stride, a.V, nullptr);
    select_row<MASK>(r, a, row);
}

template <typename T, bool MASK>
__global__ __launch_bounds__(DS_THREADS) void decode_select_block_kernel(SelectArgs a) {
    extern __shared__ __attribute__((aligned(16))) float ds_lds[];
    const int row = blockIdx.x;
    BlockRow r;
    r.load(reinterpret_cast<const T*>(a.logits) + (long)row * a.row_stride, a.V, ds_lds);
    select_row<MASK>(r, a, row);
}

// f(std::integral_constant<int, ITEMS>{}) for the smallest ladder step holding V
template <typename F>
inline void dispatch_items(int V, F&& f) {
    const int need = (V + WAVE - 1) / WAVE;
    if (need <= 1) f(std::integral_constant<int, 1>{});
    else if (need <= 2) f(std::integral_constant<int, 2>{});
    else if (need <= 4) f(std::integral_constant<int, 4>{});
    else if (need <= 8) f(std::integral_constant<int, 8>{});
    else f(std::integral_constant<int, 16>{});
}

template <typename T, bool MASK>
void launch_select(const SelectArgs& a) {
    auto stream = at::cuda::getCurrentCUDAStream();
    if (a.V <= DS_WAVE_MAXV) {
        dispatch_items(a.V, [&](auto items) {
            hipLaunchKernelGGL((decode_select_wave_kernel<T, decltype(items)::value, MASK>),
                               dim3((a.B + DS_WAVES - 1) / DS_WAVES), dim3(DS_THREADS), 0, stream,
                               a);
        });
    } else {
        const size_t smem = (size_t)((a.V + 3) & ~3) * sizeof(float) + DS_WAVES * 8;
        allow_dynamic_lds<decode_select_block_kernel<T, MASK>>(smem);
        hipLaunchKernelGGL((decode_select_block_kernel<T, MASK>), dim3(a.B), dim3(DS_THREADS),
                           smem, stream, a);
    }
    HIP_CHECK_LAST();
}

template <typename P>
const P* row_param(const torch::Tensor& t, torch::ScalarType st, long B, const torch::Tensor& like,
                   const char* name) {
    TORCH_CHECK(t.device() == like.device() && t.scalar_type() == st && t.dim() == 1 &&
                    t.size(0) == B && t.is_contiguous(),
                "decode_select: ", name, " must be a contiguous (", B, ",) tensor of the right ",
                "dtype on the logits' device");
    return t.data_ptr<P>();
}

SelectArgs common_args(const torch::Tensor& logits, const torch::Tensor& do_sample,
                       const torch::Tensor& temperature, const torch::Tensor& top_k,
                       const torch::Tensor& top_p) {
    TORCH_CHECK(logits.is_cuda() && logits.dim() == 2, "decode_select: logits must be (B, V) on the GPU");
    TORCH_CHECK(logits.scalar_type() == torch::kBFloat16 || logits.scalar_type() == torch::kFloat32,
                "decode_select: logits must be bf16 or fp32");
    const long B = logits.size(0), V = logits.size(1);
    TORCH_CHECK(B > 0 && B < (1L << 30), "decode_select: bad batch size");
    TORCH_CHECK(V >= 1 && V <= DS_BLOCK_MAXV, "decode_select: V out of range (decode_select_applicable)");
    TORCH_CHECK(logits.stride(1) == 1 || V == 1, "decode_select: the vocabulary dim must be contiguous");
    SelectArgs a = {};
    a.logits = logits.data_ptr();
    a.row_stride = logits.stride(0);
    a.B = (int)B;
    a.V = (int)V;
    a.do_sample = row_param<int>(do_sample, torch::kInt32, B, logits, "do_sample");
    a.temperature = row_param<float>(temperature, torch::kFloat32, B, logits, "temperature");
    a.top_k = row_param<int>(top_k, torch::kInt32, B, logits, "top_k");
    a.top_p = row_param<float>(top_p, torch::kFloat32, B, logits, "top_p");
    return a;
}

const long long* i64_param(const torch::Tensor& t, long n, const torch::Tensor& like,
                           const char* name) {
    TORCH_CHECK(t.device() == like.device() && t.scalar_type() == torch::kInt64 &&
                    t.numel() == n && t.is_contiguous(),
                "decode_select: ", name, " must be a contiguous int64 tensor of ", n,
                " element(s) on the logits' device");
    return reinterpret_cast<const long long*>(t.data_ptr<int64_t>());
}

}  // namespace

bool decode_select_applicable(long V) { return V >= 1 && V <= DS_BLOCK_MAXV; }

// tokens = select(logits) into `tok` (allocated when absent), with the decode
// bookkeeping for whichever of out_buf+step / done+eos_fill are passed
torch::Tensor decode_select(torch::Tensor logits, torch::Tensor do_sample,
                            torch::Tensor temperature, torch::Tensor top_k, torch::Tensor top_p,
                            torch::Tensor seed, torch::Tensor draw,
                            c10::optional<torch::Tensor> tok, c10::optional<torch::Tensor> out_buf,
                            c10::optional<torch::Tensor> step, c10::optional<torch::Tensor> done,
                            c10::optional<torch::Tensor> eos_fill) {
    SelectArgs a = common_args(logits, do_sample, temperature, top_k, top_p);
    a.seed = i64_param(seed, 1, logits, "seed");
    a.draw = i64_param(draw, 1, logits, "draw");
    torch::Tensor out;
    if (has_tensor(tok)) {
        out = *tok;
        i64_param(out, a.B, logits, "tok");
    } else {
        TORCH_CHECK(!has_tensor(out_buf), "decode_select: out_buf needs the tok buffer");
        out = torch::empty({(long)a.B}, logits.options().dtype(torch::kInt64));
    }
    a.tok = reinterpret_cast<long long*>(out.data_ptr<int64_t>());
    if (has_tensor(out_buf)) {
        TORCH_CHECK(has_tensor(step), "decode_select: out_buf needs the step cursor");
        const auto& ob = *out_buf;
        TORCH_CHECK(ob.device() == logits.device() && ob.scalar_type() == torch::kInt64 &&
                        ob.dim() == 2 && ob.size(0) == a.B && ob.stride(1) == 1,
                    "decode_select: out_buf must be (B, cols) int64 with contiguous rows");
        a.out_buf = reinterpret_cast<long long*>(ob.data_ptr<int64_t>());
        a.out_stride = ob.stride(0);
        a.out_cols = (int)ob.size(1);
        a.step = i64_param(*step, 1, logits, "step");
    }
    if (has_tensor(done)) {
        TORCH_CHECK(has_tensor(eos_fill), "decode_select: done needs eos_fill");
        const auto& d = *done;
        TORCH_CHECK(d.device() == logits.device() && d.scalar_type() == torch::kBool &&
                        d.numel() == a.B && d.is_contiguous(),
                    "decode_select: done must be a contiguous (B,) bool tensor");
        a.done = reinterpret_cast<unsigned char*>(d.data_ptr<bool>());
        a.eos_fill = i64_param(*eos_fill, 2, logits, "eos_fill");
    }
    if (logits.scalar_type() == torch::kFloat32) launch_select<float, false>(a);
    else launch_select<unsigned short, false>(a);
    return out;
}

// debug entry of the same kernel: the kept set of every row as a (B, V) bool mask
torch::Tensor decode_keep_mask(torch::Tensor logits, torch::Tensor temperature,
                               torch::Tensor top_k, torch::Tensor top_p) {
    auto ds = torch::ones({logits.size(0)}, logits.options().dtype(torch::kInt32));
    SelectArgs a = common_args(logits, ds, temperature, top_k, top_p);
    auto mask = torch::empty({(long)a.B, (long)a.V}, logits.options().dtype(torch::kBool));
    a.mask = reinterpret_cast<unsigned char*>(mask.data_ptr<bool>());
    if (logits.scalar_type() == torch::kFloat32) launch_select<float, true>(a);
    else launch_select<unsigned short, true>(a);
    return mask;
}
