// Python bindings for the perceiver_amd CDNA4 (gfx950) kernel extension.
#include <torch/extension.h>

torch::Tensor gelu_bias_fwd(torch::Tensor x, c10::optional<torch::Tensor> bias);
torch::Tensor gelu_bias_bwd(torch::Tensor x, c10::optional<torch::Tensor> bias, torch::Tensor dy);

std::vector<torch::Tensor> flash_fwd(torch::Tensor q, torch::Tensor k, torch::Tensor v,
                                     c10::optional<torch::Tensor> pad_mask, bool causal,
                                     double dropout_p, int64_t seed);
std::vector<torch::Tensor> flash_bwd(torch::Tensor dout, torch::Tensor q, torch::Tensor k,
                                     torch::Tensor v, torch::Tensor out, torch::Tensor lse,
                                     c10::optional<torch::Tensor> pad_mask, bool causal,
                                     double dropout_p, int64_t seed,
                                     c10::optional<torch::Tensor> qkv_grad);
std::vector<torch::Tensor> ln_fwd(torch::Tensor x, torch::Tensor w, c10::optional<torch::Tensor> b,
                                  double eps);
std::vector<torch::Tensor> add_ln_fwd(torch::Tensor h, torch::Tensor x, torch::Tensor w,
                                      c10::optional<torch::Tensor> b, double eps);
std::vector<torch::Tensor> ln_bwd(torch::Tensor dy, torch::Tensor x, torch::Tensor w,
                                  torch::Tensor mean, torch::Tensor rstd, bool needs_dwdb,
                                  c10::optional<torch::Tensor> ds);
bool flash_supported_impl(long d_qk, long d_v);
bool flash_bwd_packs_qkv_grad(long D, long Dv);
std::tuple<int64_t, int64_t> flash_split_plan(int64_t blocks, int64_t len, int64_t tile);
bool flash_fwd_pipe_applicable(long D, long Dv, long Nq);
void adamw_step(torch::Tensor master, torch::Tensor m, torch::Tensor v, torch::Tensor g,
                double lr, double beta1, double beta2, double eps, double weight_decay,
                int64_t step);
torch::Tensor rotary_apply(torch::Tensor t, torch::Tensor frq, int64_t rot, bool neg_sin);
torch::Tensor dropout_add_fwd(torch::Tensor x, torch::Tensor res, double p, int64_t seed);
torch::Tensor dropout_add_bwd(torch::Tensor dy, double p, int64_t seed);
torch::Tensor colsum_bf16(torch::Tensor x);
torch::Tensor gemm_bt_bf16(torch::Tensor x, torch::Tensor w, c10::optional<torch::Tensor> bias);
std::vector<torch::Tensor> gemm_bt_gelu_bf16(torch::Tensor x, torch::Tensor w,
                                             c10::optional<torch::Tensor> bias);
bool gemm_bt_applicable(long M, long N, long K);
torch::Tensor transpose_bf16(torch::Tensor x);
std::vector<torch::Tensor> gemm_wgrad(torch::Tensor dy, torch::Tensor x, bool want_db);
bool gemm_wgrad_applicable(long M, long N, long K);
std::tuple<int64_t, int64_t, int64_t, int64_t> wgrad_plan(int64_t M, int64_t N, int64_t K);
torch::Tensor decode_select(torch::Tensor logits, torch::Tensor do_sample,
                            torch::Tensor temperature, torch::Tensor top_k, torch::Tensor top_p,
                            torch::Tensor seed, torch::Tensor draw,
                            c10::optional<torch::Tensor> tok, c10::optional<torch::Tensor> out_buf,
                            c10::optional<torch::Tensor> step, c10::optional<torch::Tensor> done,
                            c10::optional<torch::Tensor> eos_fill);
torch::Tensor decode_keep_mask(torch::Tensor logits, torch::Tensor temperature,
                               torch::Tensor top_k, torch::Tensor top_p);
bool decode_select_applicable(long V);
void beam_select(torch::Tensor logits, torch::Tensor score, torch::Tensor done,
                 torch::Tensor gen_len, torch::Tensor tok, torch::Tensor src,
                 torch::Tensor all_done, torch::Tensor eos_fill, int64_t num_beams,
                 c10::optional<torch::Tensor> step, int64_t rec_offset,
                 c10::optional<torch::Tensor> rec_tok, c10::optional<torch::Tensor> rec_parent,
                 c10::optional<torch::Tensor> rec_all_done);
bool beam_select_applicable(long V, long num_beams);
void beam_reorder(torch::Tensor table, torch::Tensor counters, torch::Tensor src,
                  int64_t num_beams);
torch::Tensor decode_attn(torch::Tensor q, torch::Tensor k, torch::Tensor v,
                          c10::optional<torch::Tensor> lo, torch::Tensor hi);
bool decode_attn_applicable(long D, long Dv);
std::tuple<int64_t, int64_t> decode_attn_plan(int64_t B, int64_t H, int64_t cap, int64_t D);

bool contrastive_applicable(long V, long k, long C);
std::tuple<int64_t, int64_t> contrastive_plan(int64_t G, int64_t cap, int64_t C);
torch::Tensor contrastive_sim(torch::Tensor h, torch::Tensor hist, torch::Tensor rnorm,
                              torch::Tensor hist_len, int64_t k);
void contrastive_commit(torch::Tensor logits, torch::Tensor tok, torch::Tensor prob, int64_t k,
                        c10::optional<torch::Tensor> h, c10::optional<torch::Tensor> part,
                        c10::optional<torch::Tensor> hist, c10::optional<torch::Tensor> rnorm,
                        c10::optional<torch::Tensor> hist_len, c10::optional<torch::Tensor> done,
                        c10::optional<torch::Tensor> src, c10::optional<torch::Tensor> alpha,
                        c10::optional<torch::Tensor> eos_fill, c10::optional<torch::Tensor> step,
                        c10::optional<torch::Tensor> rec, c10::optional<torch::Tensor> sim_out,
                        c10::optional<torch::Tensor> score_out);
void contrastive_copy(torch::Tensor table, torch::Tensor counters, torch::Tensor src, int64_t k);

PYBIND11_MODULE(TORCH_EXTENSION_NAME, m) {
    m.def("gelu_bias_fwd", &gelu_bias_fwd, "fused bias+GELU forward (bf16)");
    m.def("gelu_bias_bwd", &gelu_bias_bwd, "fused bias+GELU backward (bf16)");
    m.def("flash_fwd", &flash_fwd, "fused flash attention forward");
    m.def("flash_bwd", &flash_bwd,
          "fused flash attention backward; with qkv_grad, a (B, N, 2*qk + v) bf16 buffer, dq/dk/dv "
          "are written as its column slices and returned as views of it",
          pybind11::arg("dout"), pybind11::arg("q"), pybind11::arg("k"), pybind11::arg("v"),
          pybind11::arg("out"), pybind11::arg("lse"), pybind11::arg("pad_mask"),
          pybind11::arg("causal"), pybind11::arg("dropout_p"), pybind11::arg("seed"),
          pybind11::arg("qkv_grad") = pybind11::none());
    // needs_dropout is kept for callers; dropout runs in-kernel and never narrows the gate
    m.def("flash_supported", [](int64_t d_qk, int64_t d_v, int64_t /*needs_dropout*/) {
        return flash_supported_impl(d_qk, d_v);
    }, "shape gate for the flash kernel");
    m.def("flash_bwd_packs_qkv_grad", [](int64_t d_qk, int64_t d_v) {
        return flash_bwd_packs_qkv_grad(d_qk, d_v);
    }, "host-only: whether flash_bwd accepts a packed qkv gradient buffer at these head dims");
    m.def("flash_split_plan", &flash_split_plan,
          "host-only: (nsplit, chunk) of the gridDim.z split for blocks workgroups over a len-long axis");
    m.def("flash_fwd_pipe_applicable", [](int64_t d, int64_t dv, int64_t nq) {
        return flash_fwd_pipe_applicable(d, dv, nq);
    }, "host-only: whether the pipelined forward has a template for (D, Dv) at Nq queries");
    m.def("ln_fwd", &ln_fwd, "fused bf16 LayerNorm forward");
    m.def("add_ln_fwd", &add_ln_fwd,
          "residual add + bf16 LayerNorm in one pass: returns (s = h + x, y, mean, rstd)");
    m.def("ln_bwd", &ln_bwd,
          "fused bf16 LayerNorm backward; with ds the first result is bf16(dx) + ds",
          pybind11::arg("dy"), pybind11::arg("x"), pybind11::arg("w"), pybind11::arg("mean"),
          pybind11::arg("rstd"), pybind11::arg("needs_dwdb"),
          pybind11::arg("ds") = pybind11::none());
    m.def("adamw_step", &adamw_step, "single-pass fused AdamW on flat fp32 state");
    m.def("rotary_apply", &rotary_apply, "fused rotary embedding (bf16, fwd/bwd via neg_sin)");
    m.def("dropout_add_fwd", &dropout_add_fwd, "fused residual dropout-add forward (bf16)");
    m.def("dropout_add_bwd", &dropout_add_bwd, "fused residual dropout-add backward (bf16)");
    m.def("colsum_bf16", &colsum_bf16, "coalesced bf16 column sum (bias gradients)");
    m.def("gemm_bt", &gemm_bt_bf16, "deep-pipeline bf16 GEMM: x @ w^T (+ bias)");
    m.def("transpose_bf16", &transpose_bf16, "LDS-tiled bf16 2-D transpose");
    m.def("gemm_bt_gelu", &gemm_bt_gelu_bf16,
          "deep-pipeline bf16 GEMM with fused GELU epilogue: returns (pre, gelu(pre+bias))");
    m.def("gemm_bt_applicable", [](int64_t M, int64_t N, int64_t K) {
        return gemm_bt_applicable(M, N, K);
    }, "shape gate for the custom GEMM");
    m.def("gemm_wgrad", &gemm_wgrad,
          "split-K weight gradient dy^T @ x with fused bias-gradient sums: returns (dw[, db])");
    m.def("gemm_wgrad_applicable", [](int64_t M, int64_t N, int64_t K) {
        return gemm_wgrad_applicable(M, N, K);
    }, "shape gate for the weight-gradient GEMM");
    m.def("wgrad_plan", &wgrad_plan,
          "host-only: (tile_n, tile_k, nsplit, rows_per_split) of the weight-gradient GEMM");
    m.def("decode_select", &decode_select,
          "fused decode token selection (greedy / temperature, top-k, top-p) with EOS bookkeeping",
          pybind11::arg("logits"), pybind11::arg("do_sample"), pybind11::arg("temperature"),
          pybind11::arg("top_k"), pybind11::arg("top_p"), pybind11::arg("seed"),
          pybind11::arg("draw"), pybind11::arg("tok") = pybind11::none(),
          pybind11::arg("out_buf") = pybind11::none(), pybind11::arg("step") = pybind11::none(),
          pybind11::arg("done") = pybind11::none(), pybind11::arg("eos_fill") = pybind11::none());
    m.def("decode_keep_mask", &decode_keep_mask,
          "debug entry of decode_select: the kept set of every row as a (B, V) bool mask");
    m.def("decode_select_applicable", [](int64_t V) { return decode_select_applicable(V); },
          "host-only: whether decode_select has a tier for a vocabulary of V");
    m.def("decode_attn", &decode_attn,
          "single-query attention over the per-row key windows lo[b] .. hi[b] (inclusive, int64 "
          "device tensors of 1 or B elements; lo None means 0)",
          pybind11::arg("q"), pybind11::arg("k"), pybind11::arg("v"), pybind11::arg("lo"),
          pybind11::arg("hi"));
    m.def("decode_attn_applicable",
          [](int64_t d, int64_t dv) { return decode_attn_applicable(d, dv); },
          "host-only: whether decode_attn takes these head dims");
    m.def("decode_attn_plan", &decode_attn_plan,
          "host-only: (nsplit, row granule) of decode_attn's static grid (nsplit, H, B)");
    m.def("beam_select", &beam_select,
          "one beam-search step per group of num_beams rows: top-k of score + log-softmax with "
          "done / gen_len / token / parent bookkeeping",
          pybind11::arg("logits"), pybind11::arg("score"), pybind11::arg("done"),
          pybind11::arg("gen_len"), pybind11::arg("tok"), pybind11::arg("src"),
          pybind11::arg("all_done"), pybind11::arg("eos_fill"), pybind11::arg("num_beams"),
          pybind11::arg("step") = pybind11::none(), pybind11::arg("rec_offset") = 0,
          pybind11::arg("rec_tok") = pybind11::none(),
          pybind11::arg("rec_parent") = pybind11::none(),
          pybind11::arg("rec_all_done") = pybind11::none());
    m.def("beam_select_applicable",
          [](int64_t V, int64_t num_beams) { return beam_select_applicable(V, num_beams); },
          "host-only: whether beam_select takes a vocabulary of V with num_beams beams");
    m.def("beam_reorder", &beam_reorder,
          "in-place permutation of the generated rows of every described cache buffer by the "
          "per-group source beams",
          pybind11::arg("table"), pybind11::arg("counters"), pybind11::arg("src"),
          pybind11::arg("num_beams"));
    m.def("contrastive_applicable",
          [](int64_t V, int64_t k, int64_t C) { return contrastive_applicable(V, k, C); },
          "host-only: whether the contrastive kernels take a vocabulary of V, k candidates and "
          "hidden states of C channels");
    m.def("contrastive_plan", &contrastive_plan,
          "host-only: (nsplit, row granule) of contrastive_sim's static grid (nsplit, G)");
    m.def("contrastive_sim", &contrastive_sim,
          "per slice of the history the k maxima of dot(hist_t, h_j) * rnorm_t: (nsplit, G, 8) fp32",
          pybind11::arg("h"), pybind11::arg("hist"), pybind11::arg("rnorm"),
          pybind11::arg("hist_len"), pybind11::arg("k"));
    m.def("contrastive_commit", &contrastive_commit,
          "one contrastive-search step per group of k rows: score, select, record, append to the "
          "history and propose the next k candidates; without h the proposal alone",
          pybind11::arg("logits"), pybind11::arg("tok"), pybind11::arg("prob"), pybind11::arg("k"),
          pybind11::arg("h") = pybind11::none(), pybind11::arg("part") = pybind11::none(),
          pybind11::arg("hist") = pybind11::none(), pybind11::arg("rnorm") = pybind11::none(),
          pybind11::arg("hist_len") = pybind11::none(), pybind11::arg("done") = pybind11::none(),
          pybind11::arg("src") = pybind11::none(), pybind11::arg("alpha") = pybind11::none(),
          pybind11::arg("eos_fill") = pybind11::none(), pybind11::arg("step") = pybind11::none(),
          pybind11::arg("rec") = pybind11::none(), pybind11::arg("sim_out") = pybind11::none(),
          pybind11::arg("score_out") = pybind11::none());
    m.def("contrastive_copy", &contrastive_copy,
          "copy the row at each described cache buffer's length counter from the selected row of "
          "every group to the group's other rows",
          pybind11::arg("table"), pybind11::arg("counters"), pybind11::arg("src"),
          pybind11::arg("k"));
}
