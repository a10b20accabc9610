// The taps of a dilated 1-D convolution over the frames of a clip, moved into the operand of a product (rnn_cell tcn; vltf.h,
// DESIGN 4.31).  Rows are clip-major, r = b T + t; L = min(max(seq_len[b], 0), T) live steps (seq_len NULL: T).  Tap j reads at
// offset (j - (taps - 1) / 2) dilation, or (j - (taps - 1)) dilation in the causal form.
//   fwd: cols[r][j C + c] = x[r + off_j][c] where t < L and 0 <= t + off_j < L, +0.0f everywhere else; every element is written.
//   bwd: dx[r][c] = dres[r][c] + sum over j ascending with 0 <= t - off_j < L of dcols[r - off_j][j C + c]; dead rows +0.0f.
// Both are gathers per OUTPUT element: no atomics, no LDS (a clip's T C floats are re-read `taps` times out of L2), nothing read
// where a zero is stored, so rows t >= L of x, dcols and dres may hold NaN.  A thread owns VEC consecutive columns of one row:
// VEC = 4 (16-byte loads and stores) where C % 4 == 0 and every pointer is 16-byte aligned, VEC = 1 otherwise.  Consecutive
// threads walk the taps C columns of a row, so the stores are coalesced over a row of cols.  Index arithmetic is 64-bit.
#include "common.h"

#define TC_THREADS 256
#define TC_MAX_BLOCKS 8192
#define TC_MAX_TAPS 9
#define TC_MAX_DILATION 65536
#define TC_MAX_C 1024

template <int VEC>
struct tc_vec;
template <>
struct tc_vec<1> {
    typedef float type;
    static __device__ __forceinline__ float zero() { return 0.f; }
    static __device__ __forceinline__ float add(float a, float b) { return a + b; }
};
template <>
struct tc_vec<4> {
    typedef float4 type;
    static __device__ __forceinline__ float4 zero() { return make_float4(0.f, 0.f, 0.f, 0.f); }
    static __device__ __forceinline__ float4 add(float4 a, float4 b) { return make_float4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w); }
};

__device__ __forceinline__ int tc_len(const int32_t* __restrict__ seq_len, int b, int T) {
    return seq_len ? min(max(seq_len[b], 0), T) : T;
}

// offset of tap j: j0 = (taps - 1) / 2 centred, taps - 1 causal
__device__ __forceinline__ int tc_off(int j, int j0, int dilation) { return (j - j0) * dilation; }

template <int VEC>
__global__ __launch_bounds__(TC_THREADS) void tconv_cols_fwd_kernel(const float* __restrict__ x, const int32_t* __restrict__ seq_len,
                                                                    float* __restrict__ cols, int64_t rows, int T, int C, int taps,
                                                                    int dilation, int j0) {
    typedef typename tc_vec<VEC>::type V;
    const int CV = C / VEC, WV = taps * CV;                         // vectors per row of x, of cols
    const int64_t total = rows * WV, step = (int64_t)gridDim.x * TC_THREADS;
    for (int64_t i = (int64_t)blockIdx.x * TC_THREADS + threadIdx.x; i < total; i += step) {
        const int64_t row = i / WV;
        const int w = (int)(i - row * WV), j = w / CV, cv = w - j * CV;
        const int b = (int)(row / T), t = (int)(row - (int64_t)b * T);
        const int L = tc_len(seq_len, b, T);
        const int64_t s = (int64_t)t + tc_off(j, j0, dilation);
        V v = tc_vec<VEC>::zero();
        if (t < L && s >= 0 && s < L) v = reinterpret_cast<const V*>(x)[((int64_t)b * T + s) * CV + cv];
        reinterpret_cast<V*>(cols)[i] = v;
    }
}

template <int VEC>
__global__ __launch_bounds__(TC_THREADS) void tconv_cols_bwd_kernel(const float* __restrict__ dcols, const float* __restrict__ dres,
                                                                    const int32_t* __restrict__ seq_len, float* __restrict__ dx,
                                                                    int64_t rows, int T, int C, int taps, int dilation, int j0) {
    typedef typename tc_vec<VEC>::type V;
    const int CV = C / VEC, WV = taps * CV;
    const int64_t total = rows * CV, step = (int64_t)gridDim.x * TC_THREADS;
    for (int64_t i = (int64_t)blockIdx.x * TC_THREADS + threadIdx.x; i < total; i += step) {
        const int64_t row = i / CV;
        const int cv = (int)(i - row * CV);
        const int b = (int)(row / T), t = (int)(row - (int64_t)b * T);
        const int L = tc_len(seq_len, b, T);
        V acc = tc_vec<VEC>::zero();
        if (t < L) {
            if (dres) acc = reinterpret_cast<const V*>(dres)[i];
            for (int j = 0; j < taps; ++j) {                        // ascending taps, plain adds: the order the contract states
                const int64_t s = (int64_t)t - tc_off(j, j0, dilation);
                if (s >= 0 && s < L) acc = tc_vec<VEC>::add(acc, reinterpret_cast<const V*>(dcols)[((int64_t)b * T + s) * WV + (int64_t)j * CV + cv]);
            }
        }
        reinterpret_cast<V*>(dx)[i] = acc;
    }
}

static int tc_check(const char* who, int batch, int T, int C, int taps, int dilation, int causal) {
    VL_CHECK(batch > 0 && T > 0 && C > 0, "%s: batch %d, T %d, C %d must be positive", who, batch, T, C);
    VL_CHECK(taps >= 1 && taps <= TC_MAX_TAPS, "%s: taps %d must lie in 1..%d", who, taps, TC_MAX_TAPS);
    VL_CHECK(causal || (taps & 1), "%s: taps %d must be odd unless causal (a centred kernel has a middle tap)", who, taps);
    VL_CHECK(dilation >= 1 && dilation <= TC_MAX_DILATION, "%s: dilation %d must lie in 1..%d", who, dilation, TC_MAX_DILATION);
    VL_CHECK(C <= TC_MAX_C, "%s: C %d exceeds %d", who, C, TC_MAX_C);
    return 0;
}

static inline bool tc_aligned(const void* p) { return p == nullptr || ((uintptr_t)p & 15) == 0; }

static inline int tc_blocks(int64_t total) {
    const int64_t blocks = (total + TC_THREADS - 1) / TC_THREADS;
    return (int)(blocks < TC_MAX_BLOCKS ? blocks : TC_MAX_BLOCKS);
}

extern "C" int vl_tconv_cols_fwd(const float* x, const int32_t* seq_len, float* cols, int batch, int T, int C, int taps, int dilation,
                                 int causal, vl_stream_t stream) {
    VL_CHECK(x && cols, "vl_tconv_cols_fwd: null pointer");
    if (int rc = tc_check("vl_tconv_cols_fwd", batch, T, C, taps, dilation, causal)) return rc;
    const int64_t rows = (int64_t)batch * T;
    const int j0 = causal ? taps - 1 : (taps - 1) / 2;
    if (C % 4 == 0 && tc_aligned(x) && tc_aligned(cols))
        hipLaunchKernelGGL(tconv_cols_fwd_kernel<4>, dim3(tc_blocks(rows * taps * (C / 4))), dim3(TC_THREADS), 0, (hipStream_t)stream, x,
                           seq_len, cols, rows, T, C, taps, dilation, j0);
    else
        hipLaunchKernelGGL(tconv_cols_fwd_kernel<1>, dim3(tc_blocks(rows * taps * C)), dim3(TC_THREADS), 0, (hipStream_t)stream, x,
                           seq_len, cols, rows, T, C, taps, dilation, j0);
    VL_LAUNCH_CHECK();
    return 0;
}

extern "C" int vl_tconv_cols_bwd(const float* dcols, const float* dres, const int32_t* seq_len, float* dx, int batch, int T, int C,
                                 int taps, int dilation, int causal, vl_stream_t stream) {
    VL_CHECK(dcols && dx, "vl_tconv_cols_bwd: null pointer");
    if (int rc = tc_check("vl_tconv_cols_bwd", batch, T, C, taps, dilation, causal)) return rc;
    const int64_t rows = (int64_t)batch * T;
    const int j0 = causal ? taps - 1 : (taps - 1) / 2;
    if (C % 4 == 0 && tc_aligned(dcols) && tc_aligned(dres) && tc_aligned(dx))
        hipLaunchKernelGGL(tconv_cols_bwd_kernel<4>, dim3(tc_blocks(rows * (C / 4))), dim3(TC_THREADS), 0, (hipStream_t)stream, dcols, dres,
                           seq_len, dx, rows, T, C, taps, dilation, j0);
    else
        hipLaunchKernelGGL(tconv_cols_bwd_kernel<1>, dim3(tc_blocks(rows * C)), dim3(TC_THREADS), 0, (hipStream_t)stream, dcols, dres,
                           seq_len, dx, rows, T, C, taps, dilation, j0);
    VL_LAUNCH_CHECK();
    return 0;
}
