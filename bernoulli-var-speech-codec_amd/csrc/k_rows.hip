// Row-wise utility kernels around the BVRNN GEMMs: normalisation, the natural <-> fragment-packed re-ordering, fill, strided
// row copy, and the KL term of BVRNN.forward.
#include "k_gemm.h"

namespace bvc {

// workgroups of 256 threads for a grid-stride loop over `total` elements
static int grid_stride_blocks(long long total) {
    const long long blocks = (total + 255) / 256;
    return (int)(blocks > 4096 ? 4096 : blocks);
}

__global__ void normalize_rows_kernel(const float *__restrict__ y, const float *__restrict__ mean,
                                      const float *__restrict__ stdv, long long total, int n,
                                      float *__restrict__ out) {
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total;
         i += (long long)gridDim.x * blockDim.x) {
        const int c = (int)(i % n);
        out[i] = (y[i] - mean[c]) / stdv[c];
    }
}

int launch_normalize_rows(const float *y, const float *mean, const float *stdv, long long rows, int n,
                          float *out, hipStream_t s) {
    const long long total = rows * n;
    if (total <= 0) return BVC_OK;
    hipLaunchKernelGGL(normalize_rows_kernel, dim3(grid_stride_blocks(total)), dim3(256), 0, s, y, mean, stdv, total, n, out);
    BVC_HIP_TRY(hipGetLastError());
    return BVC_OK;
}

__global__ void repack_rows_kernel(const float *__restrict__ src, float *__restrict__ dst, long long ld, int rows,
                                   int n, int dir) {
    const long long total = (long long)rows * n;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total;
         i += (long long)gridDim.x * blockDim.x) {
        const int m = (int)(i / n), c = (int)(i % n);
        if (dir == 0) dst[packed_off(m, c, n)] = src[(long long)m * ld + c];
        else          dst[(long long)m * ld + c] = src[packed_off(m, c, n)];
    }
}

int launch_repack_rows(const float *src, float *dst, long long ld_natural, int rows, int n, int dir, hipStream_t s) {
    const long long total = (long long)rows * n;
    if (total <= 0) return BVC_OK;
    hipLaunchKernelGGL(repack_rows_kernel, dim3(grid_stride_blocks(total)), dim3(256), 0, s, src, dst, ld_natural, rows, n, dir);
    BVC_HIP_TRY(hipGetLastError());
    return BVC_OK;
}

__global__ void fill_kernel(float *p, float v, long long n) {
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n;
         i += (long long)gridDim.x * blockDim.x)
        p[i] = v;
}

int launch_fill(float *p, float v, long long n, hipStream_t s) {
    if (n <= 0) return BVC_OK;
    hipLaunchKernelGGL(fill_kernel, dim3(grid_stride_blocks(n)), dim3(256), 0, s, p, v, n);
    BVC_HIP_TRY(hipGetLastError());
    return BVC_OK;
}

__global__ void copy_rows_kernel(const float *__restrict__ src, long long lds_, float *__restrict__ dst,
                                 long long ldd, int rows, int n) {
    const long long total = (long long)rows * n;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total;
         i += (long long)gridDim.x * blockDim.x) {
        const long long rr = i / n;
        const int c = (int)(i % n);
        dst[rr * ldd + c] = src[rr * lds_ + c];
    }
}

int launch_copy_rows(const float *src, long long lds_, float *dst, long long ldd, int rows, int n,
                     hipStream_t s) {
    const long long total = (long long)rows * n;
    if (total <= 0) return BVC_OK;
    hipLaunchKernelGGL(copy_rows_kernel, dim3(grid_stride_blocks(total)), dim3(256), 0, s, src, lds_, dst, ldd, rows, n);
    BVC_HIP_TRY(hipGetLastError());
    return BVC_OK;
}

// ---- KL term of BVRNN.forward ---------------------------------------------------------------------
// One workgroup per frame; thread (b, j) pairs strided, fixed-order tree reduction (deterministic).
__global__ __launch_bounds__(256) void kld_frames_kernel(const float *__restrict__ prob, const float *__restrict__ prior,
                                                         const float *__restrict__ bits, int B, long long T, int Z,
                                                         float *__restrict__ kld) {
    __shared__ float red[256];
    const long long t = blockIdx.x;
    float sum = 0.0f;
    for (int i = threadIdx.x; i < B * Z; i += 256) {
        const int b = i / Z, j = i - b * Z;
        const long long o = ((long long)b * T + t) * Z + j;
        if (bits && !(bits[(long long)b * T + t] > (float)j)) continue;        // kld_elem * bit_mask
        const float e = prob[o], q = prior[o];
        const float a = e * (logf(fmaxf(e, 1e-3f)) - logf(fmaxf(q, 1e-3f)));
        const float c = (1.0f - e) * (logf(fmaxf(1.0f - e, 1e-3f)) - logf(fmaxf(1.0f - q, 1e-3f)));
        sum += a + c;
    }
    red[threadIdx.x] = sum;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) red[threadIdx.x] += red[threadIdx.x + w];
        __syncthreads();
    }
    if (threadIdx.x == 0) kld[t] = red[0] / (float)B;
}

int launch_kld_frames(const float *prob, const float *prior, const float *bits, int B, long long T, int Z, float *kld,
                      hipStream_t s) {
    if (T <= 0) return BVC_OK;
    hipLaunchKernelGGL(kld_frames_kernel, dim3((unsigned)T), dim3(256), 0, s, prob, prior, bits, B, T, Z, kld);
    BVC_HIP_TRY(hipGetLastError());
    return BVC_OK;
}

}  // namespace bvc
