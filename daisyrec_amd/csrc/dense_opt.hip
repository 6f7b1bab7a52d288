// The dense optimisers over a flat parameter buffer (torch.optim's single-tensor math; every kernel clears the gradient
// it consumed) and the step dispatcher of the library-issued epoch loops (daisy_{neumf,nfm,vae}_fit_epoch).
#include <math.h>

#include "common.h"

namespace daisy {

__global__ __launch_bounds__(kBlock) void k_sgd_dense(float *__restrict__ W, float *__restrict__ g, int64_t n,
                                                      float lr) {
    for (int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; e < n; e += (int64_t)gridDim.x * blockDim.x) {
        W[e] = fmaf(-lr, g[e], W[e]);
        g[e] = 0.f;
    }
}

// torch.optim.Adam single-tensor math (exp_avg.lerp_, addcmul_, addcdiv_), dense
__global__ __launch_bounds__(kBlock) void k_adam_dense(float *__restrict__ W, float *__restrict__ g,
                                                       float *__restrict__ m, float *__restrict__ v,
                                                       int64_t n, float step_size, float beta1,
                                                       float beta2, float eps, float bc2_sqrt) {
    const float w1 = 1.f - beta1, w2 = 1.f - beta2;
    for (int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; e < n;
         e += (int64_t)gridDim.x * blockDim.x) {
        const float gg = g[e];
        const float mm = fmaf(w1, gg - m[e], m[e]);          // lerp(m, g, 1-beta1)
        const float vv = fmaf(w2 * gg, gg, beta2 * v[e]);    // mul_(beta2).addcmul_(g,g,1-beta2)
        const float denom = sqrtf(vv) / bc2_sqrt + eps;
        W[e] = W[e] - step_size * (mm / denom);
        m[e] = mm;
        v[e] = vv;
        g[e] = 0.f;
    }
}

// torch.optim.Adagrad single-tensor math (defaults): state_sum.addcmul_(g, g); w.addcdiv_(g, sqrt(state_sum) + eps, -lr)
__global__ __launch_bounds__(kBlock) void k_adagrad_dense(float *__restrict__ W, float *__restrict__ g,
                                                          float *__restrict__ ss, int64_t n, float lr, float eps) {
    for (int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; e < n; e += (int64_t)gridDim.x * blockDim.x) {
        const float gg = g[e];
        const float s2 = fmaf(gg, gg, ss[e]);
        W[e] = W[e] - lr * (gg / (sqrtf(s2) + eps));
        ss[e] = s2;
        g[e] = 0.f;
    }
}

// torch.optim.RMSprop single-tensor math (defaults): sq.mul_(alpha).addcmul_(g, g, 1-alpha); w.addcdiv_(g, sqrt(sq) + eps, -lr)
__global__ __launch_bounds__(kBlock) void k_rmsprop_dense(float *__restrict__ W, float *__restrict__ g,
                                                          float *__restrict__ sq, int64_t n, float lr, float alpha,
                                                          float eps) {
    const float w2 = 1.f - alpha;
    for (int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; e < n; e += (int64_t)gridDim.x * blockDim.x) {
        const float gg = g[e];
        const float s2 = fmaf(w2 * gg, gg, alpha * sq[e]);
        W[e] = W[e] - lr * (gg / (sqrtf(s2) + eps));
        sq[e] = s2;
        g[e] = 0.f;
    }
}

int dense_opt_check(const char *what, int32_t optimizer, const float *state0, const float *state1) {
    DAISY_CHECK_ARG(optimizer >= 0 && optimizer <= 3, "%s: optimizer=%d (0 sgd, 1 adam, 2 adagrad, 3 rmsprop)", what, optimizer);
    DAISY_CHECK_ARG(optimizer == 0 || state0, "%s: optimizer %d needs its state", what, optimizer);
    DAISY_CHECK_ARG(optimizer != 1 || state1, "%s: Adam needs both moments", what);
    return DAISY_OK;
}

int dense_opt_step(int32_t optimizer, float *W, float *g, float *state0, float *state1, int64_t n, float lr, int64_t t,
                   daisy_stream_t stream) {
    if (optimizer == 0) return daisy_sgd_dense(W, g, n, lr, stream);
    if (optimizer == 1) return daisy_adam_dense(W, g, state0, state1, n, lr, 0.9f, 0.999f, 1e-8f, t, stream);
    if (optimizer == 2) return daisy_adagrad_dense(W, g, state0, n, lr, 1e-10f, stream);
    return daisy_rmsprop_dense(W, g, state0, n, lr, 0.99f, 1e-8f, stream);
}

}  // namespace daisy

using namespace daisy;

extern "C" {

int daisy_sgd_dense(float *W, float *g, int64_t n, float lr, daisy_stream_t stream) {
    DAISY_CHECK_ARG(W && g && n > 0, "sgd_dense: bad argument");
    hipLaunchKernelGGL(k_sgd_dense, dim3(grid_for(n, kBlock * 4)), dim3(kBlock), 0, as_stream(stream), W, g, n, lr);
    DAISY_LAUNCH_CHECK();
    return DAISY_OK;
}

int daisy_adam_dense(float *W, float *g, float *m, float *v, int64_t n, float lr, float beta1,
                     float beta2, float eps, int64_t step, daisy_stream_t stream) {
    DAISY_CHECK_ARG(W && g && m && v && n > 0 && step >= 1, "adam_dense: bad argument");
    const double bc1 = 1.0 - pow((double)beta1, (double)step);
    const double bc2 = 1.0 - pow((double)beta2, (double)step);
    hipLaunchKernelGGL(k_adam_dense, dim3(grid_for(n, kBlock * 4)), dim3(kBlock), 0, as_stream(stream), W, g, m,
                       v, n, (float)((double)lr / bc1), beta1, beta2, eps, (float)sqrt(bc2));
    DAISY_LAUNCH_CHECK();
    return DAISY_OK;
}

int daisy_adagrad_dense(float *W, float *g, float *state_sum, int64_t n, float lr, float eps, daisy_stream_t stream) {
    DAISY_CHECK_ARG(W && g && state_sum && n > 0, "adagrad_dense: bad argument");
    hipLaunchKernelGGL(k_adagrad_dense, dim3(grid_for(n, kBlock * 4)), dim3(kBlock), 0, as_stream(stream), W, g, state_sum, n, lr,
                       eps);
    DAISY_LAUNCH_CHECK();
    return DAISY_OK;
}

int daisy_rmsprop_dense(float *W, float *g, float *square_avg, int64_t n, float lr, float alpha, float eps,
                        daisy_stream_t stream) {
    DAISY_CHECK_ARG(W && g && square_avg && n > 0, "rmsprop_dense: bad argument");
    hipLaunchKernelGGL(k_rmsprop_dense, dim3(grid_for(n, kBlock * 4)), dim3(kBlock), 0, as_stream(stream), W, g, square_avg, n,
                       lr, alpha, eps);
    DAISY_LAUNCH_CHECK();
    return DAISY_OK;
}

}  // extern "C"
