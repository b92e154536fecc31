// BN recalibration (liburso_train.so; recalibrate_bn, Config.BN_RECAL_BATCHES): the exact, momentum-free pooling of
// the float32 batch statistics that the batch-statistics forward pass leaves on the device into float64 population statistics, and their
// settlement into the statistics buffer.  Rule, table layout and argument rules: include/ursonet_train.h; ursonet_amd/bn_recal.py is the
// same rule in NumPy float64.
//
// Both launches: a channel is one thread's (no atomics, no exchange), blockIdx.y strides over the layers of the table and blockIdx.x over a
// layer's channels, so any grid gives the same bits.  A few thousand channels in all: the launches are latency, not bandwidth.
#include "../csrc/common.h"
#include "../../include/ursonet_train.h"

static constexpr int RECAL_T = 256;                                         // threads per block
static constexpr int RECAL_MAX_L = 65535;                                   // gridDim.y
static constexpr int64_t RECAL_MAX_PIXELS = (int64_t)1 << 53;               // t * M stays an exact double

// One more batch into channel (mean, m2): five statements, every float64 operation rounded once (-ffp-contract=off).
__device__ __forceinline__ void recal_add_one(double& mean, double& m2, double mu_b, double v_b, double n, double M) {
    const double n1 = n + M;
    const double d = mu_b - mean;
    const double dm = d * M;
    const double step = dm / n1;
    const double vm = v_b * M;
    const double dd = d * d;
    const double nm = n * M;
    const double w = nm / n1;
    const double between = dd * w;
    const double add = vm + between;
    mean = mean + step;
    m2 = m2 + add;
}

__global__ void __launch_bounds__(RECAL_T) bn_recal_add_kernel(int L, const urso_bn_recal_layer* __restrict__ layers, double* __restrict__ acc, int64_t t) {
    for (int l = blockIdx.y; l < L; l += gridDim.y) {
        const urso_bn_recal_layer y = layers[l];
        const double M = (double)y.M, n = (double)(t * y.M);
        double* __restrict__ mean = acc + y.off_mean;
        double* __restrict__ m2 = acc + y.off_var;
        for (int64_t c = (int64_t)blockIdx.x * RECAL_T + threadIdx.x; c < y.N; c += (int64_t)gridDim.x * RECAL_T) {
            double a = mean[c], b = m2[c];
            recal_add_one(a, b, (double)y.bmean[c], (double)y.bvar[c], n, M);
            mean[c] = a;
            m2[c] = b;
        }
    }
}

__global__ void __launch_bounds__(RECAL_T) bn_recal_settle_kernel(int L, const urso_bn_recal_layer* __restrict__ layers, const double* __restrict__ acc,
                                                                  float* __restrict__ stats, int64_t t) {
    for (int l = blockIdx.y; l < L; l += gridDim.y) {
        const urso_bn_recal_layer y = layers[l];
        const double n = (double)(t * y.M);
        for (int64_t c = (int64_t)blockIdx.x * RECAL_T + threadIdx.x; c < y.N; c += (int64_t)gridDim.x * RECAL_T) {
            const double var = acc[y.off_var + c] / n;
            stats[y.off_mean + c] = (float)acc[y.off_mean + c];
            stats[y.off_var + c] = (float)var;
        }
    }
}

// ------------------------------------------------------------------------------------------------ host
// The refusals all three entry points begin with; tmax: the largest t the launch multiplies M with (< 0: none).  Returns the widest layer.
static int64_t recal_refuse(const char* fn, int L, const urso_bn_recal_layer* h, int64_t n_stats, const void* layers_d, int64_t tmax) {
    if (L <= 0 || L > RECAL_MAX_L) { urso_set_error("%s: L must be in [1, %d] (got %d)", fn, RECAL_MAX_L, L); return -1; }
    if (!h || !layers_d) { urso_set_error("%s: null pointer (layers_h, layers_d)", fn); return -1; }
    if (((uintptr_t)layers_d) & 7) { urso_set_error("%s: layers_d must be 8-byte aligned", fn); return -1; }
    if (n_stats <= 0) { urso_set_error("%s: n_stats must be > 0 (got %lld)", fn, (long long)n_stats); return -1; }
    int64_t widest = 0;
    for (int l = 0; l < L; ++l) {
        const urso_bn_recal_layer& y = h[l];
        if (!y.bmean || !y.bvar) { urso_set_error("%s: layer %d: null pointer (bmean, bvar)", fn, l); return -1; }
        if ((((uintptr_t)y.bmean) | ((uintptr_t)y.bvar)) & 3) { urso_set_error("%s: layer %d: bmean and bvar must be 4-byte aligned", fn, l); return -1; }
        if (y.N <= 0) { urso_set_error("%s: layer %d: N must be > 0 (got %lld)", fn, l, (long long)y.N); return -1; }
        if (y.M <= 0) { urso_set_error("%s: layer %d: M must be > 0 (got %lld)", fn, l, (long long)y.M); return -1; }
        if (y.off_mean < 0 || y.off_var < 0) { urso_set_error("%s: layer %d: negative offset", fn, l); return -1; }
        if (y.N > n_stats || y.off_mean > n_stats - y.N || y.off_var > n_stats - y.N) {
            urso_set_error("%s: layer %d: a slice ends behind n_stats = %lld", fn, l, (long long)n_stats); return -1;
        }
        if (tmax >= 0 && tmax > RECAL_MAX_PIXELS / y.M) { urso_set_error("%s: layer %d: t * M exceeds 2^53", fn, l); return -1; }
        widest = y.N > widest ? y.N : widest;
    }
    // the 2 L slices, pairwise disjoint (L is a few dozen: the plain double loop)
    for (int a = 0; a < 2 * L; ++a)
        for (int b = a + 1; b < 2 * L; ++b) {
            const int64_t oa = (a & 1) ? h[a >> 1].off_var : h[a >> 1].off_mean, na = h[a >> 1].N;
            const int64_t ob = (b & 1) ? h[b >> 1].off_var : h[b >> 1].off_mean, nb = h[b >> 1].N;
            if (oa < ob + nb && ob < oa + na) { urso_set_error("%s: the slices of layers %d and %d overlap", fn, a >> 1, b >> 1); return -1; }
        }
    return widest;
}

static dim3 recal_grid(int L, int64_t widest) {
    const int64_t bx = (widest + RECAL_T - 1) / RECAL_T;
    return dim3((unsigned)(bx > 64 ? 64 : bx), (unsigned)L);
}

extern "C" int urso_bn_recal_plan(int L, const urso_bn_recal_layer* layers_h, int64_t n_stats, urso_bn_recal_layer* layers_d) {
    const char* fn = "urso_bn_recal_plan";
    if (recal_refuse(fn, L, layers_h, n_stats, layers_d, -1) < 0) return URSO_EINVAL;
    const hipError_t e = hipMemcpy(layers_d, layers_h, (size_t)L * sizeof(urso_bn_recal_layer), hipMemcpyHostToDevice);
    if (e != hipSuccess) { urso_set_error("%s: copying the table: %s", fn, hipGetErrorString(e)); return URSO_ELAUNCH; }
    return URSO_OK;
}

extern "C" int urso_bn_recal_add(int L, const urso_bn_recal_layer* layers_h, const urso_bn_recal_layer* layers_d, int64_t n_stats, double* acc_d,
                                 int64_t t, void* stream) {
    const char* fn = "urso_bn_recal_add";
    if (t < 0) { urso_set_error("%s: t must be >= 0 (got %lld)", fn, (long long)t); return URSO_EINVAL; }
    if (t == INT64_MAX) { urso_set_error("%s: t * M exceeds 2^53", fn); return URSO_EINVAL; }
    const int64_t widest = recal_refuse(fn, L, layers_h, n_stats, layers_d, t + 1);
    if (widest < 0) return URSO_EINVAL;
    if (!acc_d) { urso_set_error("%s: null pointer (acc)", fn); return URSO_EINVAL; }
    if (((uintptr_t)acc_d) & 7) { urso_set_error("%s: acc must be 8-byte aligned", fn); return URSO_EINVAL; }
    hipStream_t st = (hipStream_t)stream;
    ProfScope ps(st, URSO_K_OPTIM, 0, 0.0);
    URSO_KLAUNCH(bn_recal_add_kernel, recal_grid(L, widest), dim3(RECAL_T), 0, st, L, layers_d, acc_d, t);
    return urso_check_launch(fn);
}

extern "C" int urso_bn_recal_settle(int L, const urso_bn_recal_layer* layers_h, const urso_bn_recal_layer* layers_d, int64_t n_stats,
                                    const double* acc_d, float* stats_d, int64_t t, void* stream) {
    const char* fn = "urso_bn_recal_settle";
    if (t < 1) { urso_set_error("%s: nothing was added: t must be >= 1 (got %lld)", fn, (long long)t); return URSO_EINVAL; }
    const int64_t widest = recal_refuse(fn, L, layers_h, n_stats, layers_d, t);
    if (widest < 0) return URSO_EINVAL;
    if (!acc_d || !stats_d) { urso_set_error("%s: null pointer (acc, stats)", fn); return URSO_EINVAL; }
    if (((uintptr_t)acc_d) & 7) { urso_set_error("%s: acc must be 8-byte aligned", fn); return URSO_EINVAL; }
    if (((uintptr_t)stats_d) & 3) { urso_set_error("%s: stats must be 4-byte aligned", fn); return URSO_EINVAL; }
    hipStream_t st = (hipStream_t)stream;
    ProfScope ps(st, URSO_K_OPTIM, 0, 0.0);
    URSO_KLAUNCH(bn_recal_settle_kernel, recal_grid(L, widest), dim3(RECAL_T), 0, st, L, layers_d, acc_d, stats_d, t);
    return urso_check_launch(fn);
}
