// bfhip_wave_probe.hip -- bfhip_wave_sum_probe: the sampler kernels' 64-lane sums (bfhip_wave.h) on given lane values, in
// the form the library was built with and in the packed and the unpacked form by name, so that a test can compare the forms
// bit for bit with each other and with an emulation of the instruction's lane maps (tests/test_gpu_wave_sum.py).
// bfhip_wave_packs_probe: the same sums left in their vector registers (wave_sum_packs), read value by value, and the test the
// U-turn checks take on them in place (tests/test_gpu_wave_packs.py).
#include "bfhip_common.h"
#include "bfhip_wave.h"

// one wave per batch: in[(batch * N + i) * 64 + lane] -> out[batch * N + i]
template <int N>
__global__ __launch_bounds__(64) void bf_wave_sum_probe_kernel(int form, const double *__restrict__ in, double *__restrict__ out) {
    const int lane = threadIdx.x;
    const size_t base = (size_t)blockIdx.x * N;
    double v[N];
#pragma unroll
    for (int i = 0; i < N; ++i) v[i] = in[(base + i) * 64 + lane];
    if (form == BFHIP_WSUM_PACKED) wave_sum_n_packed<N>(v);
    else if (form == BFHIP_WSUM_UNPACKED) wave_sum_n_unpacked<N>(v);
    else wave_sum_n<N>(v);
    if (lane == 0) {
#pragma unroll
        for (int i = 0; i < N; ++i) out[base + i] = v[i];
    }
}

template <int N>
static void wave_sum_probe_launch(bfhip_ctx *ctx, int n_batch, int form, const double *in, double *out) {
    hipLaunchKernelGGL(bf_wave_sum_probe_kernel<N>, dim3((unsigned)n_batch), dim3(64), 0, ctx->stream, form, in, out);
}

extern "C" int bfhip_wave_sum_probe(bfhip_ctx *ctx, int n_batch, int n_val, int form, const double *in, double *out) {
    BfDeviceGuard dev_guard(ctx);
    if (!ctx || n_batch < 0 || n_val < 1 || n_val > BFHIP_WSUM_MAX || form < BFHIP_WSUM_BUILT || form > BFHIP_WSUM_UNPACKED ||
        (n_batch > 0 && (!in || !out)))
        return bf_set_error(BFHIP_ERR_ARG, "bfhip_wave_sum_probe: invalid argument");
    if (n_batch == 0) return 0;
    switch (n_val) {
        case 1: wave_sum_probe_launch<1>(ctx, n_batch, form, in, out); break;
        case 2: wave_sum_probe_launch<2>(ctx, n_batch, form, in, out); break;
        case 3: wave_sum_probe_launch<3>(ctx, n_batch, form, in, out); break;
        case 4: wave_sum_probe_launch<4>(ctx, n_batch, form, in, out); break;
        case 5: wave_sum_probe_launch<5>(ctx, n_batch, form, in, out); break;
        case 6: wave_sum_probe_launch<6>(ctx, n_batch, form, in, out); break;
        default: wave_sum_probe_launch<7>(ctx, n_batch, form, in, out); break;
    }
    BF_HIP_CHECK(hipGetLastError());
    return 0;
}

// one wave per batch: in[(batch * N + i) * 64 + lane] -> out[batch * N + i] through get(i), flag[batch] = any_le0()
template <int N>
__global__ __launch_bounds__(64) void bf_wave_packs_probe_kernel(const double *__restrict__ in, double *__restrict__ out, int *__restrict__ flag) {
    const int lane = threadIdx.x;
    const size_t base = (size_t)blockIdx.x * N;
    double v[N];
#pragma unroll
    for (int i = 0; i < N; ++i) v[i] = in[(base + i) * 64 + lane];
    const WavePacks<N> pk = wave_sum_packs<N>(v);
    const bool le0 = pk.any_le0();
#pragma unroll
    for (int i = 0; i < N; ++i) v[i] = pk.get(i);
    if (lane == 0) {
#pragma unroll
        for (int i = 0; i < N; ++i) out[base + i] = v[i];
        flag[blockIdx.x] = le0 ? 1 : 0;
    }
}

template <int N>
static void wave_packs_probe_launch(bfhip_ctx *ctx, int n_batch, const double *in, double *out, int *flag) {
    hipLaunchKernelGGL(bf_wave_packs_probe_kernel<N>, dim3((unsigned)n_batch), dim3(64), 0, ctx->stream, in, out, flag);
}

extern "C" int bfhip_wave_packs_probe(bfhip_ctx *ctx, int n_batch, int n_val, const double *in, double *out, int *flag) {
    BfDeviceGuard dev_guard(ctx);
    if (!ctx || n_batch < 0 || n_val < 1 || n_val > BFHIP_WSUM_MAX || (n_batch > 0 && (!in || !out || !flag)))
        return bf_set_error(BFHIP_ERR_ARG, "bfhip_wave_packs_probe: invalid argument");
    if (n_batch == 0) return 0;
    switch (n_val) {
        case 1: wave_packs_probe_launch<1>(ctx, n_batch, in, out, flag); break;
        case 2: wave_packs_probe_launch<2>(ctx, n_batch, in, out, flag); break;
        case 3: wave_packs_probe_launch<3>(ctx, n_batch, in, out, flag); break;
        case 4: wave_packs_probe_launch<4>(ctx, n_batch, in, out, flag); break;
        case 5: wave_packs_probe_launch<5>(ctx, n_batch, in, out, flag); break;
        case 6: wave_packs_probe_launch<6>(ctx, n_batch, in, out, flag); break;
        default: wave_packs_probe_launch<7>(ctx, n_batch, in, out, flag); break;
    }
    BF_HIP_CHECK(hipGetLastError());
    return 0;
}
