// Support kernels of the persistent recurrence (k_flow.hip): the residency census, the sentinel fill, the one-kernel preparation of
// a launch, the device copy of its arguments.
#include "bvc_internal.h"

namespace bvc {

// Residency census (bvc_model_create): are `gridDim.x` workgroups with the recurrence kernels' footprint - 512 threads, every
// VGPR of the compute unit, the filler kernels' LDS - resident at once?  Every workgroup adds itself to ctr[0] and waits
// (bounded) until all have; ctr[1] counts those that gave up.  A kernel of its own, so that no profile mixes it with the
// recurrence launches.
__global__ __launch_bounds__(512, 2) void flow_census_kernel(unsigned *ctr, unsigned spin_limit) {
    asm volatile("; the recurrence kernels' register footprint" ::: "v255");
    if (threadIdx.x == 0) {
        __hip_atomic_fetch_add(ctr, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        unsigned spins = 0;
        while (__hip_atomic_load(ctr, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < gridDim.x) {
            __builtin_amdgcn_s_sleep(8);
            if (++spins > spin_limit) {                    // bounded: a workgroup queued behind a resident one never lets the count complete
                __hip_atomic_fetch_add(ctr + 1, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                break;
            }
        }
    }
}

// the device copy of a launch's arguments, by the threads of one workgroup
static_assert(sizeof(FlowArgs) % 4 == 0, "FlowArgs is copied in dwords");
__device__ __forceinline__ void flow_copy_args(FlowArgs *dst, const FlowArgs &v) {
    const unsigned *src = reinterpret_cast<const unsigned *>(&v);
    unsigned *d = reinterpret_cast<unsigned *>(dst);
    for (unsigned i = threadIdx.x; i < sizeof(FlowArgs) / 4; i += blockDim.x) d[i] = src[i];
}

// workgroups of 256 threads for a grid-stride loop over n elements (k_rows.hip's grid_stride_blocks allows twice as many)
static int flow_fill_blocks(long long n) {
    const long long blocks = (n + 255) / 256;
    return (int)(blocks > 2048 ? 2048 : blocks);
}

__global__ void fill_u32_kernel(unsigned *p, unsigned v, long long n) {
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) p[i] = v;
}

// Everything a persistent launch needs in place, as ONE kernel: the flow region filled with the sentinel, its first buffer - h of frame -1:
// n_h0 = mt16 * H floats in operand-fragment order - set to the caller's initial state (natural (B, H) rows; null: zero; padding rows
// zero), and the device copy of the arguments.
__global__ __launch_bounds__(256) void flow_prepare_kernel(FlowArgs *dst, FlowArgs v, unsigned *flow, long long n_flow, long long n_h0,
                                                           const float *__restrict__ h0, int B, int H) {
    if (blockIdx.x == 0) flow_copy_args(dst, v);
    const int ntile = H >> 4;
    uint4 *flow4 = reinterpret_cast<uint4 *>(flow);
    const long long n4 = n_flow >> 2, h4 = n_h0 >> 2;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (long long)gridDim.x * blockDim.x) {
        uint4 o = {FLOW_POISON, FLOW_POISON, FLOW_POISON, FLOW_POISON};
        if (i < h4) {                                      // 16 bytes of a fragment-packed block: columns n .. n + 3 of row m
            const long long tile = i >> 6;
            const int lane = (int)(i & 63);
            const int m = (int)(tile / ntile) * 16 + (lane & 15), n = (int)(tile % ntile) * 16 + (lane >> 4) * 4;
            float4 hv = {0.f, 0.f, 0.f, 0.f};
            if (h0 && m < B) hv = *reinterpret_cast<const float4 *>(h0 + (long long)m * H + n);
            o = {__float_as_uint(hv.x), __float_as_uint(hv.y), __float_as_uint(hv.z), __float_as_uint(hv.w)};
        }
        flow4[i] = o;
    }
}

int launch_flow_prepare(const FlowArgs &a, FlowArgs *d_args, unsigned *flow, long long n_flow, long long n_h0, const float *d_h0, int B, int H,
                        hipStream_t s) {
    if (n_flow % 4 || n_h0 % 4 || H % 16 || n_h0 > n_flow || (d_h0 && (reinterpret_cast<uintptr_t>(d_h0) & 15))) {
        set_error("flow_prepare: unaligned flow region or initial state");
        return BVC_EINVAL;
    }
    const int grid = flow_fill_blocks(n_flow / 4);
    hipLaunchKernelGGL(flow_prepare_kernel, dim3(grid > 0 ? grid : 1), dim3(256), 0, s, d_args, a, flow, n_flow, n_h0, d_h0, B, H);
    BVC_HIP_TRY(hipGetLastError());
    return BVC_OK;
}

int launch_fill_u32(unsigned *p, unsigned v, long long n, hipStream_t s) {
    if (n <= 0) return BVC_OK;
    hipLaunchKernelGGL(fill_u32_kernel, dim3(flow_fill_blocks(n)), dim3(256), 0, s, p, v, n);
    BVC_HIP_TRY(hipGetLastError());
    return BVC_OK;
}

// the census asks for the LDS of the largest single-chain form (the filler kernels'); allowed where the persistent kernels' are
// (flow_kernels_init)
int flow_census_init() {
    BVC_HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void *>(flow_census_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)FlowLds<8>::bytes(FF_FILL)));
    return BVC_OK;
}

int launch_flow_census(unsigned *ctr, int grid, unsigned spin_limit, hipStream_t s) {
    hipLaunchKernelGGL(flow_census_kernel, dim3(grid), dim3(512), FlowLds<8>::bytes(FF_FILL), s, ctr, spin_limit);
    BVC_HIP_TRY(hipGetLastError());
    return BVC_OK;
}

__global__ void flow_set_args_kernel(FlowArgs *dst, FlowArgs v) { flow_copy_args(dst, v); }

int launch_flow_set_args(const FlowArgs &a, FlowArgs *d_args, hipStream_t s) {
    hipLaunchKernelGGL(flow_set_args_kernel, dim3(1), dim3(256), 0, s, d_args, a);
    BVC_HIP_TRY(hipGetLastError());
    return BVC_OK;
}

}  // namespace bvc
