// PyTorch-ROCm custom-op surface of the C ABI (BASELINE.json north_star: "surfaced to Python through
// PyTorch-ROCm custom ops"; SURVEY.md section 8b: "registered as torch ops on the HIP dispatch key").
//
// A SHIM with no logic of its own: every op checks its tensors (device, dtype, contiguity), takes raw device
// pointers and the current HIP stream, and calls the extern "C" entry point of libdaisyrec_hip.so named in its
// comment.  Tensors are borrowed, tables are mutated in place on the current stream (SURVEY 8b "Ownership").
// Registered under the CUDA dispatch key, which IS the HIP key in a ROCm build of PyTorch; there is no CPU
// kernel, so calling an op with host tensors fails in the dispatcher ("no kernel for CPU backend").
//
//   torch.ops.daisyrec.mf_predict(P, Q, u, i)                               daisy_mf_predict       MFRecommender.py:63-68
//   torch.ops.daisyrec.mf_rank_topk(P, Q, us, cands, topk)                  daisy_mf_rank_topk     MFRecommender.py:106-123
//   torch.ops.daisyrec.mf_full_rank(P, Q, u, topk)                          daisy_mf_full_rank     MFRecommender.py:126-133
//   torch.ops.daisyrec.sample_uniform_neg(indptr, items, I, num_ng, seed, epoch)
//                                                                           daisy_sample_neg_per_user   sampler.py:82-89
//   torch.ops.daisyrec.bpr_mf_step(P, Q, u, i, j, lr, reg_1, reg_2, gamma, loss_type)
//                                                                           daisy_bpr_set_batch + daisy_bpr_sgd_step
//                                                                           AbstractRecommender.py:119-128
//   torch.ops.daisyrec.ngcf_layer_fwd(E, X, W1, b1, W2, b2, mess_p, seed, layer) -> (Y, norm)
//                                                                           daisy_ngcf_layer_forward  NGCFRecommender.py:38-60,163-167
//   torch.ops.daisyrec.ngcf_layer_bwd(dY, Y, norm, E, X, W1, W2, mess_p, seed, layer) -> (dE, dX, dW1, db1, dW2, db2)
//                                                                           daisy_ngcf_layer_backward + daisy_ngcf_wgrad_reduce
//                                                                           (dE without A_hat^T dX: the caller's sparse product)
//   torch.ops.daisyrec.nfm_scores(P, Q, ub, ib, bias, wp, W, b, bn_w, bn_b, running_mean, running_var, users, items, C, n,
//                                 act) -> scores                            daisy_nfm_scores (eval mode)  NFMRecommender.py:110-209
//   torch.ops.daisyrec.vae_scores(W, row_ptr, col, val, users, items, hidden, latent_dim, item_num) -> scores
//                                                                           daisy_vae_scores (eval mode)  VAECFRecommender.py:79-145
//   torch.ops.daisyrec.{ease,slim,knn,psvd}_full_rank_users(model operands, users, excl_indptr, excl_items, topk) -> (ids, scores)
//                                                                           daisy_{ease,slim,knn,psvd}_full_rank_users (no counterpart:
//                                                                           full ranking of many users)
#include <ATen/ATen.h>
#include <c10/core/DeviceGuard.h>
#include <c10/hip/HIPStream.h>
#include <torch/library.h>

#include <map>
#include <mutex>
#include <tuple>
#include <vector>

#include "../../include/daisyrec_amd.h"

namespace {

void need(const at::Tensor &t, at::ScalarType dt, const char *name) {
    TORCH_CHECK(t.is_cuda(), name, ": expected a HIP device tensor (there is no CPU fallback)");
    TORCH_CHECK(t.scalar_type() == dt, name, ": expected dtype ", dt, ", got ", t.scalar_type());
    TORCH_CHECK(t.is_contiguous(), name, ": tensor must be contiguous");
}

// every tensor of an op lives on the device of its first one; that device becomes the current one for the call, so
// the library's allocations (contexts), at::empty workspaces and kernel launches all land there
void same_device(const at::Tensor &first, std::initializer_list<const at::Tensor *> rest, const char *op) {
    for (const at::Tensor *t : rest)
        TORCH_CHECK(t->device() == first.device(), op, ": all tensors must be on one device (", first.device(), " vs ",
                    t->device(), ")");
}

void ok(int rc) { TORCH_CHECK(rc == DAISY_OK, "daisyrec: ", daisy_last_error()); }

daisy_stream_t stream_of(const at::Tensor &t) {
    return reinterpret_cast<daisy_stream_t>(c10::hip::getCurrentHIPStream(t.get_device()).stream());
}

at::Tensor mf_predict(const at::Tensor &P, const at::Tensor &Q, const at::Tensor &u, const at::Tensor &i) {
    need(P, at::kFloat, "P"); need(Q, at::kFloat, "Q"); need(u, at::kLong, "u"); need(i, at::kLong, "i");
    TORCH_CHECK(P.dim() == 2 && Q.dim() == 2 && P.size(1) == Q.size(1) && u.numel() == i.numel(), "mf_predict: shapes");
    same_device(P, {&Q, &u, &i}, "mf_predict");
    const c10::OptionalDeviceGuard guard(P.device());
    at::Tensor out = at::empty({u.numel()}, P.options());
    if (u.numel() == 0) return out;
    ok(daisy_mf_predict(P.data_ptr<float>(), Q.data_ptr<float>(), (int32_t)P.size(1), u.data_ptr<int64_t>(),
                        i.data_ptr<int64_t>(), u.numel(), out.data_ptr<float>(), stream_of(P)));
    return out;
}

at::Tensor mf_rank_topk(const at::Tensor &P, const at::Tensor &Q, const at::Tensor &us, const at::Tensor &cands,
                        int64_t topk) {
    need(P, at::kFloat, "P"); need(Q, at::kFloat, "Q"); need(us, at::kLong, "us"); need(cands, at::kLong, "cands");
    TORCH_CHECK(cands.dim() == 2 && us.numel() == cands.size(0), "mf_rank_topk: cands must be [len(us), C]");
    same_device(P, {&Q, &us, &cands}, "mf_rank_topk");
    const c10::OptionalDeviceGuard guard(P.device());
    const int64_t B = cands.size(0), C = cands.size(1);
    topk = topk < C ? topk : C;                                  // rank_list[:, :topk] truncates
    at::Tensor out = at::empty({B, topk}, cands.options());
    const size_t wb = daisy_mf_rank_workspace_bytes(B, C);
    at::Tensor ws = at::empty({(int64_t)(wb > 256 ? wb : 256)}, P.options().dtype(at::kByte));
    ok(daisy_mf_rank_topk(P.data_ptr<float>(), Q.data_ptr<float>(), (int32_t)P.size(1), us.data_ptr<int64_t>(),
                          cands.data_ptr<int64_t>(), B, C, (int32_t)topk, out.data_ptr<int64_t>(), nullptr,
                          ws.data_ptr(), (size_t)ws.numel(), stream_of(P)));
    return out;
}

at::Tensor mf_full_rank(const at::Tensor &P, const at::Tensor &Q, int64_t u, int64_t topk) {
    need(P, at::kFloat, "P"); need(Q, at::kFloat, "Q");
    same_device(P, {&Q}, "mf_full_rank");
    const c10::OptionalDeviceGuard guard(P.device());
    const int64_t I = Q.size(0);
    topk = topk < I ? topk : I;
    at::Tensor out = at::empty({topk}, P.options().dtype(at::kLong));
    const size_t wb = daisy_mf_full_rank_workspace_bytes(I);
    at::Tensor ws = at::empty({(int64_t)(wb > 256 ? wb : 256)}, P.options().dtype(at::kByte));
    ok(daisy_mf_full_rank(P.data_ptr<float>(), Q.data_ptr<float>(), (int32_t)P.size(1), I, u, (int32_t)topk,
                          out.data_ptr<int64_t>(), ws.data_ptr(), (size_t)ws.numel(), stream_of(P)));
    return out;
}

at::Tensor sample_uniform_neg(const at::Tensor &indptr, const at::Tensor &items, int64_t item_num, int64_t num_ng,
                              int64_t seed, int64_t epoch) {
    need(indptr, at::kLong, "indptr"); need(items, at::kInt, "items");
    same_device(items, {&indptr}, "sample_uniform_neg");
    const c10::OptionalDeviceGuard guard(items.device());
    const int64_t U = indptr.numel() - 1;
    at::Tensor js = at::empty({U, num_ng}, items.options());
    ok(daisy_sample_neg_per_user(indptr.data_ptr<int64_t>(), items.data_ptr<int32_t>(), U, item_num, (int32_t)num_ng,
                                 (uint64_t)seed, (uint64_t)epoch, js.data_ptr<int32_t>(), stream_of(items)));
    return js;
}

// per-(device, shape) training contexts of bpr_mf_step: the scratch a step needs lives in a daisy_bpr_ctx
struct CtxEntry {
    daisy_bpr_ctx *ctx;
    at::Tensor gQ, stats;
};
std::mutex g_mu;
std::map<std::tuple<int, int64_t, int64_t, int64_t, int64_t>, CtxEntry> g_ctx;

at::Tensor bpr_mf_step(at::Tensor P, at::Tensor Q, const at::Tensor &u, const at::Tensor &i, const at::Tensor &j,
                       double lr, double reg_1, double reg_2, double gamma, int64_t loss_type) {
    need(P, at::kFloat, "P"); need(Q, at::kFloat, "Q");
    need(u, at::kInt, "u"); need(i, at::kInt, "i"); need(j, at::kInt, "j");
    TORCH_CHECK(P.dim() == 2 && Q.dim() == 2 && P.size(1) == Q.size(1), "bpr_mf_step: tables must be [rows, d]");
    const int64_t B = u.numel();
    TORCH_CHECK(B > 0 && i.numel() == B && j.numel() == B, "bpr_mf_step: u, i, j must have the same length");
    same_device(P, {&Q, &u, &i, &j}, "bpr_mf_step");
    const c10::OptionalDeviceGuard guard(P.device());
    int64_t cap = 256;
    while (cap < B) cap *= 2;
    CtxEntry *e;
    {
        std::lock_guard<std::mutex> lock(g_mu);
        auto key = std::make_tuple((int)P.get_device(), cap, P.size(1), P.size(0), Q.size(0));
        auto it = g_ctx.find(key);
        if (it == g_ctx.end()) {
            CtxEntry n;
            ok(daisy_bpr_ctx_create(&n.ctx, cap, (int32_t)P.size(1), P.size(0), Q.size(0)));
            n.gQ = at::zeros_like(Q);
            n.stats = at::zeros({DAISY_STATS_LEN}, P.options().dtype(at::kDouble));
            it = g_ctx.emplace(key, n).first;
        }
        e = &it->second;
    }
    daisy_stream_t s = stream_of(P);
    ok(daisy_bpr_ctx_set_pointwise(e->ctx, loss_type >= DAISY_LOSS_CL));
    ok(daisy_bpr_set_batch(e->ctx, u.data_ptr<int32_t>(), i.data_ptr<int32_t>(), j.data_ptr<int32_t>(), B, s));
    ok(daisy_bpr_ctx_validate_batch(e->ctx, s));                 // the reference raises IndexError here
    ok(daisy_bpr_ctx_invalidate_cache(e->ctx));                  // P may have been changed by other ops between calls
    at::Tensor loss = at::empty({}, P.options().dtype(at::kDouble));
    ok(daisy_bpr_sgd_step(e->ctx, P.data_ptr<float>(), Q.data_ptr<float>(), (int32_t)loss_type, (float)gamma, (float)lr,
                          (float)reg_1, (float)reg_2, e->gQ.data_ptr<float>(), e->stats.data_ptr<double>(), nullptr,
                          loss.data_ptr<double>(), DAISY_ITEM_FUSED, s));
    return loss;
}

std::tuple<at::Tensor, at::Tensor> ngcf_layer_fwd(const at::Tensor &E, const at::Tensor &X, const at::Tensor &W1,
                                                  const at::Tensor &b1, const at::Tensor &W2, const at::Tensor &b2,
                                                  double mess_p, int64_t seed, int64_t layer) {
    for (auto *t : {&E, &X, &W1, &b1, &W2, &b2}) need(*t, at::kFloat, "ngcf_layer_fwd");
    TORCH_CHECK(E.dim() == 2 && X.sizes() == E.sizes() && W1.dim() == 2 && W1.sizes() == W2.sizes() &&
                    W1.size(1) == E.size(1) && b1.numel() == W1.size(0) && b2.numel() == W1.size(0),
                "ngcf_layer_fwd: shapes");
    same_device(E, {&X, &W1, &b1, &W2, &b2}, "ngcf_layer_fwd");
    const c10::OptionalDeviceGuard guard(E.device());
    at::Tensor Y = at::empty({E.size(0), W1.size(0)}, E.options());
    at::Tensor norm = at::empty({E.size(0)}, E.options());
    ok(daisy_ngcf_layer_forward(E.data_ptr<float>(), E.size(1), X.data_ptr<float>(), W1.data_ptr<float>(),
                                b1.data_ptr<float>(), W2.data_ptr<float>(), b2.data_ptr<float>(), Y.data_ptr<float>(),
                                Y.size(1), norm.data_ptr<float>(), E.size(0), (int32_t)E.size(1), (int32_t)Y.size(1),
                                (float)mess_p, (uint64_t)seed, (int32_t)layer, stream_of(E)));
    return {Y, norm};
}

std::tuple<at::Tensor, at::Tensor, at::Tensor, at::Tensor, at::Tensor, at::Tensor> ngcf_layer_bwd(
    const at::Tensor &dY, const at::Tensor &Y, const at::Tensor &norm, const at::Tensor &E, const at::Tensor &X,
    const at::Tensor &W1, const at::Tensor &W2, double mess_p, int64_t seed, int64_t layer) {
    for (auto *t : {&dY, &Y, &norm, &E, &X, &W1, &W2}) need(*t, at::kFloat, "ngcf_layer_bwd");
    TORCH_CHECK(E.dim() == 2 && X.sizes() == E.sizes() && W1.dim() == 2 && W1.sizes() == W2.sizes() &&
                    W1.size(1) == E.size(1) && Y.dim() == 2 && Y.size(0) == E.size(0) && Y.size(1) == W1.size(0) &&
                    dY.sizes() == Y.sizes() && norm.numel() == E.size(0),
                "ngcf_layer_bwd: shapes");
    same_device(E, {&dY, &Y, &norm, &X, &W1, &W2}, "ngcf_layer_bwd");
    const c10::OptionalDeviceGuard guard(E.device());
    const int64_t n = E.size(0);
    const int32_t din = (int32_t)E.size(1), dout = (int32_t)Y.size(1);
    at::Tensor dE = at::empty_like(E), dX = at::empty_like(E);
    at::Tensor dW1 = at::zeros_like(W1), dW2 = at::zeros_like(W2);
    at::Tensor db1 = at::zeros({dout}, E.options()), db2 = at::zeros({dout}, E.options());
    const size_t wsb = daisy_ngcf_ws_bytes(n, din, dout);
    TORCH_CHECK(wsb > 0, "ngcf_layer_bwd: unsupported widths ", din, " -> ", dout);
    at::Tensor ws = at::empty({(int64_t)wsb}, E.options().dtype(at::kByte));
    daisy_stream_t s = stream_of(E);
    ok(daisy_ngcf_layer_backward(dY.data_ptr<float>(), dout, Y.data_ptr<float>(), dout, norm.data_ptr<float>(),
                                 E.data_ptr<float>(), din, X.data_ptr<float>(), W1.data_ptr<float>(), W2.data_ptr<float>(),
                                 nullptr, 0, dE.data_ptr<float>(), dX.data_ptr<float>(), (float *)ws.data_ptr(), n, din,
                                 dout, (float)mess_p, (uint64_t)seed, (int32_t)layer, s));
    ok(daisy_ngcf_wgrad_reduce((const float *)ws.data_ptr(), n, din, dout, dW1.data_ptr<float>(), db1.data_ptr<float>(),
                               dW2.data_ptr<float>(), db2.data_ptr<float>(), s));
    return {dE, dX, dW1, db1, dW2, db2};
}

// NFM.forward in eval mode (running statistics, no dropout) over n pairs: C > 0: (users[e / C], items[e]); items absent:
// (users[0], e); C == 0: (users[e], items[e]).  W / b: the deep layers' Linear weights and biases; bn_w / bn_b /
// running_mean / running_var: one entry per stage (FM_layers first) or all empty (batch_norm off).
at::Tensor nfm_scores(const at::Tensor &P, const at::Tensor &Q, const at::Tensor &ub, const at::Tensor &ib, const at::Tensor &bias,
                      const at::Tensor &wp, at::TensorList W, at::TensorList b, at::TensorList bn_w, at::TensorList bn_b,
                      at::TensorList rmean, at::TensorList rvar, const at::Tensor &users, const c10::optional<at::Tensor> &items,
                      int64_t C, int64_t n, int64_t act) {
    for (auto *t : {&P, &Q, &ub, &ib, &bias, &wp}) need(*t, at::kFloat, "nfm_scores");
    need(users, at::kLong, "users");
    TORCH_CHECK(P.dim() == 2 && Q.dim() == 2 && P.size(1) == Q.size(1), "nfm_scores: shapes of P, Q");
    const int64_t d = P.size(1), L = (int64_t)W.size();
    TORCH_CHECK(L <= DAISY_NFM_MAX_LAYERS && b.size() == W.size(), "nfm_scores: W / b: at most ", DAISY_NFM_MAX_LAYERS, " layers");
    const bool bn = bn_w.size() > 0;
    TORCH_CHECK(!bn || ((int64_t)bn_w.size() == L + 1 && bn_b.size() == bn_w.size() && rmean.size() == bn_w.size() &&
                        rvar.size() == bn_w.size()),
                "nfm_scores: BatchNorm lists need one entry per stage (num_layers + 1)");
    same_device(P, {&Q, &ub, &ib, &bias, &wp, &users}, "nfm_scores");
    const c10::OptionalDeviceGuard guard(P.device());
    daisy_nfm_params p{};
    p.P = P.data_ptr<float>(); p.Q = Q.data_ptr<float>(); p.ub = ub.data_ptr<float>(); p.ib = ib.data_ptr<float>();
    p.bias = bias.data_ptr<float>(); p.wp = wp.data_ptr<float>();
    for (int64_t l = 0; l < L; ++l) {
        need(W[l], at::kFloat, "W"); need(b[l], at::kFloat, "b");
        TORCH_CHECK(W[l].numel() == d * d && b[l].numel() == d, "nfm_scores: layer shapes");
        p.W[l] = W[l].data_ptr<float>(); p.b[l] = b[l].data_ptr<float>();
    }
    daisy_nfm_bn_state st{};
    for (size_t k = 0; bn && k < bn_w.size(); ++k) {
        for (const at::Tensor *t : {&bn_w[k], &bn_b[k], &rmean[k], &rvar[k]}) {
            need(*t, at::kFloat, "BatchNorm");
            TORCH_CHECK(t->numel() == d, "nfm_scores: BatchNorm shapes");
        }
        p.bn_w[k] = bn_w[k].data_ptr<float>(); p.bn_b[k] = bn_b[k].data_ptr<float>();
        st.mean[k] = rmean[k].data_ptr<float>(); st.var[k] = rvar[k].data_ptr<float>();
    }
    const int64_t *ip = nullptr;
    if (items.has_value() && items->defined()) {
        need(*items, at::kLong, "items");
        n = items->numel();
        ip = items->data_ptr<int64_t>();
    }
    daisy_nfm_ctx *ctx = nullptr;
    ok(daisy_nfm_ctx_create(&ctx, 1, (int32_t)d, (int32_t)L, (int32_t)act, bn ? 1 : 0, P.size(0), Q.size(0)));
    at::Tensor out = at::empty({n}, P.options());
    const int rc = daisy_nfm_scores(ctx, &p, bn ? &st : nullptr, users.data_ptr<int64_t>(), ip, n, C, 0, 0.f, 0,
                                    out.data_ptr<float>(), stream_of(P));
    daisy_nfm_ctx_destroy(ctx);
    ok(rc);
    return out;
}

// VAECF.forward in eval mode over the users' history rows (CSR: row_ptr int64, col int32, val float32; W: the flat
// parameter buffer, encoder.0.weight item-major): [B][C] for candidates items [B][C], or [B][item_num] without them.
at::Tensor vae_scores(const at::Tensor &W, const at::Tensor &row_ptr, const at::Tensor &col, const at::Tensor &val,
                      const at::Tensor &users, const c10::optional<at::Tensor> &items, at::IntArrayRef hidden,
                      int64_t latent_dim, int64_t item_num) {
    need(W, at::kFloat, "W"); need(row_ptr, at::kLong, "row_ptr"); need(col, at::kInt, "col"); need(val, at::kFloat, "val");
    need(users, at::kLong, "users");
    TORCH_CHECK(row_ptr.dim() == 1 && row_ptr.numel() >= 2 && col.numel() == val.numel(), "vae_scores: CSR shapes");
    TORCH_CHECK((int64_t)hidden.size() <= DAISY_VAE_MAX_HIDDEN, "vae_scores: at most ", DAISY_VAE_MAX_HIDDEN, " hidden layers");
    same_device(W, {&row_ptr, &col, &val, &users}, "vae_scores");
    const c10::OptionalDeviceGuard guard(W.device());
    const int64_t U = row_ptr.numel() - 1, B = users.numel();
    TORCH_CHECK(B >= 1, "vae_scores: no users");
    TORCH_CHECK(users.min().item<int64_t>() >= 0 && users.max().item<int64_t>() < U, "vae_scores: user id out of range");
    const int64_t entries = (row_ptr.index_select(0, users + 1) - row_ptr.index_select(0, users)).sum().item<int64_t>();
    std::vector<int32_t> hid(hidden.begin(), hidden.end());
    int64_t C = 0;
    const int64_t *ip = nullptr;
    if (items.has_value() && items->defined()) {
        need(*items, at::kLong, "items");
        TORCH_CHECK(items->dim() == 2 && items->size(0) == B, "vae_scores: items must be [B, C]");
        TORCH_CHECK(items->numel() == 0 || (items->min().item<int64_t>() >= 0 && items->max().item<int64_t>() < item_num),
                    "vae_scores: item id out of range");
        C = items->size(1);
        ip = items->data_ptr<int64_t>();
    }
    daisy_vae_ctx *ctx = nullptr;
    ok(daisy_vae_ctx_create(&ctx, B, entries > 0 ? entries : 1, item_num, (int32_t)hid.size(), hid.data(), (int32_t)latent_dim));
    const int64_t need_params = daisy_vae_param_count(ctx);
    if (need_params != W.numel()) {
        daisy_vae_ctx_destroy(ctx);
        TORCH_CHECK(false, "vae_scores: W holds ", W.numel(), " floats, the layer widths need ", need_params);
    }
    at::Tensor out = at::empty({B, ip ? C : item_num}, W.options());
    const int rc = daisy_vae_scores(ctx, W.data_ptr<float>(), row_ptr.data_ptr<int64_t>(), col.data_ptr<int32_t>(),
                                    val.data_ptr<float>(), U, users.data_ptr<int64_t>(), B, entries, ip, C, nullptr, nullptr, 0,
                                    0.f, 0, out.data_ptr<float>(), stream_of(W));
    daisy_vae_ctx_destroy(ctx);
    ok(rc);
    return out;
}

// ---- full ranking of many users on fp64 scores -> (ids int64 [n, topk], scores [n, topk])
struct ExclPtrs {
    const int64_t *indptr = nullptr;
    const int32_t *items = nullptr;
};
ExclPtrs exclusion_of(const c10::optional<at::Tensor> &indptr, const c10::optional<at::Tensor> &items, const at::Tensor &first,
                      int64_t user_num, const char *op) {
    ExclPtrs e;
    const bool a = indptr.has_value() && indptr->defined(), b = items.has_value() && items->defined();
    TORCH_CHECK(a == b, op, ": excl_indptr and excl_items are given together or not at all");
    if (!a) return e;
    need(*indptr, at::kLong, "excl_indptr"); need(*items, at::kInt, "excl_items");
    same_device(first, {&*indptr, &*items}, op);
    TORCH_CHECK(indptr->numel() == user_num + 1, op, ": excl_indptr has ", indptr->numel(), " entries, expected ", user_num + 1);
    TORCH_CHECK(items->numel() >= 1, op, ": excl_items is empty (pass no exclusion instead)");
    e.indptr = indptr->data_ptr<int64_t>();
    e.items = items->data_ptr<int32_t>();
    return e;
}
void csr_of(const at::Tensor &ptr, const at::Tensor &idx, const at::Tensor &val, const char *op) {
    need(ptr, at::kLong, "ptr"); need(idx, at::kInt, "idx"); need(val, at::kFloat, "val");
    TORCH_CHECK(ptr.dim() == 1 && ptr.numel() >= 2 && idx.numel() == val.numel() && idx.numel() >= 1, op, ": CSR shapes");
}

std::tuple<at::Tensor, at::Tensor> ease_full_rank_users(const at::Tensor &row_ptr, const at::Tensor &col, const at::Tensor &val,
                                                        const at::Tensor &W, const at::Tensor &users,
                                                        const c10::optional<at::Tensor> &excl_indptr,
                                                        const c10::optional<at::Tensor> &excl_items, int64_t topk) {
    const char *op = "ease_full_rank_users";
    csr_of(row_ptr, col, val, op);
    need(W, at::kDouble, "W"); need(users, at::kLong, "users");
    TORCH_CHECK(W.dim() == 2 && W.size(0) == W.size(1), op, ": W must be square");
    same_device(W, {&row_ptr, &col, &val, &users}, op);
    const c10::OptionalDeviceGuard guard(W.device());
    const int64_t U = row_ptr.numel() - 1, n = users.numel();
    const ExclPtrs e = exclusion_of(excl_indptr, excl_items, W, U, op);
    at::Tensor ids = at::empty({n, topk}, users.options()), scores = at::empty({n, topk}, W.options());
    ok(daisy_ease_full_rank_users(row_ptr.data_ptr<int64_t>(), col.data_ptr<int32_t>(), val.data_ptr<float>(), W.data_ptr<double>(),
                                  U, W.size(0), n ? users.data_ptr<int64_t>() : nullptr, n, e.indptr, e.items, (int32_t)topk,
                                  n ? ids.data_ptr<int64_t>() : nullptr, n ? scores.data_ptr<double>() : nullptr, stream_of(W)));
    return {ids, scores};
}

std::tuple<at::Tensor, at::Tensor> slim_full_rank_users(const at::Tensor &row_ptr, const at::Tensor &col, const at::Tensor &val,
                                                        const at::Tensor &w_ptr, const at::Tensor &w_row, const at::Tensor &w_val,
                                                        const at::Tensor &users, const c10::optional<at::Tensor> &excl_indptr,
                                                        const c10::optional<at::Tensor> &excl_items, int64_t topk) {
    const char *op = "slim_full_rank_users";
    csr_of(row_ptr, col, val, op); csr_of(w_ptr, w_row, w_val, op);
    need(users, at::kLong, "users");
    same_device(val, {&row_ptr, &col, &w_ptr, &w_row, &w_val, &users}, op);
    const c10::OptionalDeviceGuard guard(val.device());
    const int64_t U = row_ptr.numel() - 1, I = w_ptr.numel() - 1, n = users.numel();
    const ExclPtrs e = exclusion_of(excl_indptr, excl_items, val, U, op);
    at::Tensor ids = at::empty({n, topk}, users.options()), scores = at::empty({n, topk}, val.options());
    ok(daisy_slim_full_rank_users(row_ptr.data_ptr<int64_t>(), col.data_ptr<int32_t>(), val.data_ptr<float>(), U, I,
                                  w_ptr.data_ptr<int64_t>(), w_row.data_ptr<int32_t>(), w_val.data_ptr<float>(),
                                  n ? users.data_ptr<int64_t>() : nullptr, n, e.indptr, e.items, (int32_t)topk,
                                  n ? ids.data_ptr<int64_t>() : nullptr, n ? scores.data_ptr<float>() : nullptr,
                                  DAISY_SLIM_PATH_AUTO, stream_of(val)));
    return {ids, scores};
}

std::tuple<at::Tensor, at::Tensor> knn_full_rank_users(const at::Tensor &l_ptr, const at::Tensor &l_col, const at::Tensor &l_val,
                                                       int64_t inner, const at::Tensor &r_ptr, const at::Tensor &r_row,
                                                       const at::Tensor &r_val, const at::Tensor &users,
                                                       const c10::optional<at::Tensor> &excl_indptr,
                                                       const c10::optional<at::Tensor> &excl_items, int64_t topk) {
    const char *op = "knn_full_rank_users";
    csr_of(l_ptr, l_col, l_val, op); csr_of(r_ptr, r_row, r_val, op);
    need(users, at::kLong, "users");
    same_device(l_val, {&l_ptr, &l_col, &r_ptr, &r_row, &r_val, &users}, op);
    const c10::OptionalDeviceGuard guard(l_val.device());
    const int64_t U = l_ptr.numel() - 1, I = r_ptr.numel() - 1, n = users.numel();
    const ExclPtrs e = exclusion_of(excl_indptr, excl_items, l_val, U, op);
    at::Tensor ids = at::empty({n, topk}, users.options()), scores = at::empty({n, topk}, l_val.options().dtype(at::kDouble));
    ok(daisy_knn_full_rank_users(l_ptr.data_ptr<int64_t>(), l_col.data_ptr<int32_t>(), l_val.data_ptr<float>(), U, inner,
                                 r_ptr.data_ptr<int64_t>(), r_row.data_ptr<int32_t>(), r_val.data_ptr<float>(), I,
                                 n ? users.data_ptr<int64_t>() : nullptr, n, e.indptr, e.items, (int32_t)topk,
                                 n ? ids.data_ptr<int64_t>() : nullptr, n ? scores.data_ptr<double>() : nullptr,
                                 DAISY_SLIM_PATH_AUTO, stream_of(l_val)));
    return {ids, scores};
}

std::tuple<at::Tensor, at::Tensor> psvd_full_rank_users(const at::Tensor &user_vec, const at::Tensor &item_vec,
                                                        const at::Tensor &users, const c10::optional<at::Tensor> &excl_indptr,
                                                        const c10::optional<at::Tensor> &excl_items, int64_t topk) {
    const char *op = "psvd_full_rank_users";
    need(user_vec, at::kDouble, "user_vec"); need(item_vec, at::kDouble, "item_vec"); need(users, at::kLong, "users");
    TORCH_CHECK(user_vec.dim() == 2 && item_vec.dim() == 2 && user_vec.size(1) == item_vec.size(1), op, ": factor counts differ");
    same_device(user_vec, {&item_vec, &users}, op);
    const c10::OptionalDeviceGuard guard(user_vec.device());
    const int64_t U = user_vec.size(0), n = users.numel();
    const ExclPtrs e = exclusion_of(excl_indptr, excl_items, user_vec, U, op);
    at::Tensor ids = at::empty({n, topk}, users.options()), scores = at::empty({n, topk}, user_vec.options());
    ok(daisy_psvd_full_rank_users(user_vec.data_ptr<double>(), item_vec.data_ptr<double>(), U, item_vec.size(0),
                                  (int32_t)user_vec.size(1), n ? users.data_ptr<int64_t>() : nullptr, n, e.indptr, e.items,
                                  (int32_t)topk, n ? ids.data_ptr<int64_t>() : nullptr, n ? scores.data_ptr<double>() : nullptr,
                                  stream_of(user_vec)));
    return {ids, scores};
}

// ---- masked top-k over rows of fp32 scores -> (ids int64 [m, topk], scores fp32 [m, topk]); scores'
// rows are contiguous, its stride is the pitch
std::tuple<at::Tensor, at::Tensor> rank_rows_f32(const at::Tensor &scores, const c10::optional<at::Tensor> &row_users,
                                                 const c10::optional<at::Tensor> &excl_indptr,
                                                 const c10::optional<at::Tensor> &excl_items, int64_t topk) {
    const char *op = "rank_rows_f32";
    TORCH_CHECK(scores.is_cuda(), "scores: expected a HIP device tensor (there is no CPU fallback)");
    TORCH_CHECK(scores.scalar_type() == at::kFloat && scores.dim() == 2, op, ": scores must be a 2-D float32 tensor");
    const int64_t m = scores.size(0), I = scores.size(1);
    TORCH_CHECK(I >= 1 && (I == 1 || scores.stride(1) == 1) && (m <= 1 || scores.stride(0) >= I), op,
                ": the rows of scores must be contiguous and must not overlap");
    const c10::OptionalDeviceGuard guard(scores.device());
    const int64_t *ru = nullptr;
    ExclPtrs e;
    if (excl_indptr.has_value() && excl_indptr->defined()) {
        TORCH_CHECK(row_users.has_value() && row_users->defined(), op, ": an exclusion needs row_users");
        e = exclusion_of(excl_indptr, excl_items, scores, excl_indptr->numel() - 1, op);
    } else {
        e = exclusion_of(excl_indptr, excl_items, scores, 0, op);
    }
    if (row_users.has_value() && row_users->defined()) {
        need(*row_users, at::kLong, "row_users");
        same_device(scores, {&*row_users}, op);
        TORCH_CHECK(row_users->numel() == m, op, ": row_users has ", row_users->numel(), " entries for ", m, " rows");
        if (m && e.indptr) ru = row_users->data_ptr<int64_t>();
    }
    const int64_t pitch = m > 1 ? scores.stride(0) : I;
    at::Tensor ids = at::empty({m, topk}, scores.options().dtype(at::kLong)), out = at::empty({m, topk}, scores.options());
    ok(daisy_rank_rows_f32(m ? scores.data_ptr<float>() : nullptr, m, I, pitch, ru, e.indptr, e.items, (int32_t)topk,
                           m ? ids.data_ptr<int64_t>() : nullptr, m ? out.data_ptr<float>() : nullptr, stream_of(scores)));
    return {ids, out};
}

}  // namespace

TORCH_LIBRARY(daisyrec, m) {
    m.def("mf_predict(Tensor P, Tensor Q, Tensor u, Tensor i) -> Tensor");
    m.def("mf_rank_topk(Tensor P, Tensor Q, Tensor us, Tensor cands, int topk) -> Tensor");
    m.def("mf_full_rank(Tensor P, Tensor Q, int u, int topk) -> Tensor");
    m.def("sample_uniform_neg(Tensor indptr, Tensor items, int item_num, int num_ng, int seed, int epoch) -> Tensor");
    m.def("bpr_mf_step(Tensor(a!) P, Tensor(b!) Q, Tensor u, Tensor i, Tensor j, float lr, float reg_1, float reg_2, "
          "float gamma, int loss_type) -> Tensor");
    m.def("ngcf_layer_fwd(Tensor E, Tensor X, Tensor W1, Tensor b1, Tensor W2, Tensor b2, float mess_p, int seed, "
          "int layer) -> (Tensor, Tensor)");
    m.def("ngcf_layer_bwd(Tensor dY, Tensor Y, Tensor norm, Tensor E, Tensor X, Tensor W1, Tensor W2, float mess_p, "
          "int seed, int layer) -> (Tensor, Tensor, Tensor, Tensor, Tensor, Tensor)");
    m.def("nfm_scores(Tensor P, Tensor Q, Tensor ub, Tensor ib, Tensor bias, Tensor wp, Tensor[] W, Tensor[] b, "
          "Tensor[] bn_w, Tensor[] bn_b, Tensor[] running_mean, Tensor[] running_var, Tensor users, Tensor? items, int C, "
          "int n, int act) -> Tensor");
    m.def("vae_scores(Tensor W, Tensor row_ptr, Tensor col, Tensor val, Tensor users, Tensor? items, int[] hidden, "
          "int latent_dim, int item_num) -> Tensor");
    m.def("ease_full_rank_users(Tensor row_ptr, Tensor col, Tensor val, Tensor W, Tensor users, Tensor? excl_indptr, "
          "Tensor? excl_items, int topk) -> (Tensor, Tensor)");
    m.def("slim_full_rank_users(Tensor row_ptr, Tensor col, Tensor val, Tensor w_ptr, Tensor w_row, Tensor w_val, Tensor users, "
          "Tensor? excl_indptr, Tensor? excl_items, int topk) -> (Tensor, Tensor)");
    m.def("knn_full_rank_users(Tensor l_ptr, Tensor l_col, Tensor l_val, int inner, Tensor r_ptr, Tensor r_row, Tensor r_val, "
          "Tensor users, Tensor? excl_indptr, Tensor? excl_items, int topk) -> (Tensor, Tensor)");
    m.def("psvd_full_rank_users(Tensor user_vec, Tensor item_vec, Tensor users, Tensor? excl_indptr, Tensor? excl_items, "
          "int topk) -> (Tensor, Tensor)");
    m.def("rank_rows_f32(Tensor scores, Tensor? row_users, Tensor? excl_indptr, Tensor? excl_items, int topk) -> "
          "(Tensor, Tensor)");
}

TORCH_LIBRARY_IMPL(daisyrec, CUDA, m) {      // the CUDA dispatch key is the HIP key of a ROCm build
    m.impl("mf_predict", &mf_predict);
    m.impl("mf_rank_topk", &mf_rank_topk);
    m.impl("mf_full_rank", &mf_full_rank);
    m.impl("sample_uniform_neg", &sample_uniform_neg);
    m.impl("bpr_mf_step", &bpr_mf_step);
    m.impl("ngcf_layer_fwd", &ngcf_layer_fwd);
    m.impl("ngcf_layer_bwd", &ngcf_layer_bwd);
    m.impl("nfm_scores", &nfm_scores);
    m.impl("vae_scores", &vae_scores);
    m.impl("ease_full_rank_users", &ease_full_rank_users);
    m.impl("slim_full_rank_users", &slim_full_rank_users);
    m.impl("knn_full_rank_users", &knn_full_rank_users);
    m.impl("psvd_full_rank_users", &psvd_full_rank_users);
    m.impl("rank_rows_f32", &rank_rows_f32);
}
