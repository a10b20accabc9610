// Multi-head self-attention over the frames of a clip (rnn_cell mhsa; vltf.h).
// One workgroup of SA_THREADS per (clip, head), no atomics, every sum in one fixed order: what a workgroup writes is a function of its
// clip's inputs alone, so a clip's bits are the same alone or in any batch.  With L = min(max(seq_len[b], 0), T) live steps (NULL: T),
// rows t >= L of qkv and dctx are never read.  The problems are tiny (about 65 kFLOP at T = 16, dh = 64) and latency-bound: the
// products run on the vector ALU out of LDS, not on the matrix pipe.
//
// LDS (dynamic: up to 3 x 64 x 129 + 64 x 65 floats = 113 KB forward, above the 64 KB static limit): the head's tiles [T][dhp] with
// dhp = dh | 1 -- an ODD row stride, so that the lanes of a half-wave, which walk the KEYS of K (or V in the backward's dP), fall on
// different banks at every d (ds_read_b32 banks are dword address % 32; dh itself is 32-, 64- or 128-aligned at the common shapes and
// would put all 32 lanes on one bank).  The odd stride also separates the two or four query rows a half-wave spans when T < 32.  The
// score tile is [T][T + 1].
#include "common.h"

#define SA_THREADS 256
#define SA_WAVES (SA_THREADS / 64)
#define SA_MAX_T 64
#define SA_MAX_H 1024
#define SA_MIN_DH 8
#define SA_MAX_DH 128

__device__ __forceinline__ int sa_len(const int32_t* __restrict__ seq_len, int b, int T) {
    return seq_len ? min(max(seq_len[b], 0), T) : T;
}

static inline int sa_dhp(int dh) { return dh | 1; }
static inline size_t sa_fwd_lds(int T, int dh) { return sizeof(float) * ((size_t)3 * T * sa_dhp(dh) + (size_t)T * (T + 1)); }
static inline size_t sa_bwd_lds(int T, int dh) { return sizeof(float) * ((size_t)2 * T * sa_dhp(dh) + (size_t)2 * T * (T + 1)); }

// the live rows of one of the head's three tiles: block 0 = Q, 1 = K, 2 = V of qkv's row [3H] (or block 0 of a [H]-wide tensor)
__device__ __forceinline__ void sa_stage(float* __restrict__ tile, const float* __restrict__ src, int64_t row0, int ld, int col0, int L,
                                         int dh, int dhp, int tid) {
    for (int idx = tid; idx < L * dh; idx += SA_THREADS) {
        const int t = idx / dh, d = idx - t * dh;
        tile[t * dhp + d] = src[(row0 + t) * ld + col0 + d];
    }
}

// DROP (vl_mhsa_drop_fwd): P is stored UNDROPPED, and the thread that stores element (q, k) puts P M / keep back into the
// score tile, from which ctx is formed: one more barrier, the same LDS.  The draw's counter is the element's index in the P of the
// whole batch, (((clip0 + b) heads + h) T + q) T + k.  Without DROP the kernel is what it was, instruction for instruction.
template <bool DROP>
__global__ __launch_bounds__(SA_THREADS) void mhsa_fwd_kernel(const float* __restrict__ qkv, const float* __restrict__ pos,
                                                              const int32_t* __restrict__ seq_len, float* __restrict__ P,
                                                              float* __restrict__ ctx, int T, int H, int heads, int dh, float scale,
                                                              float keep, uint32_t salt, SaDraw dw) {
    extern __shared__ __attribute__((aligned(16))) float sa_lds[];
    const int b = blockIdx.x / heads, h = blockIdx.x - b * heads;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int L = sa_len(seq_len, b, T), dhp = dh | 1, SP = T + 1;
    float* Q = sa_lds;
    float* K = Q + T * dhp;
    float* V = K + T * dhp;
    float* S = V + T * dhp;
    const int64_t row0 = (int64_t)b * T;
    sa_stage(Q, qkv, row0, 3 * H, h * dh, L, dh, dhp, tid);
    sa_stage(K, qkv, row0, 3 * H, H + h * dh, L, dh, dhp, tid);
    sa_stage(V, qkv, row0, 3 * H, 2 * H + h * dh, L, dh, dhp, tid);
    __syncthreads();
    // scores of the live pairs: a thread per (q, k), lanes over k, d ascending
    const float* pb = pos ? pos + (int64_t)h * (2 * T - 1) + (T - 1) : nullptr;
    for (int idx = tid; idx < L * L; idx += SA_THREADS) {
        const int q = idx / L, k = idx - q * L;
        const float* qr = Q + q * dhp;
        const float* kr = K + k * dhp;
        float acc = 0.f;
        for (int d = 0; d < dh; ++d) acc = __fmaf_rn(qr[d], kr[d], acc);
        acc *= scale;
        if (pb) acc += pb[k - q];
        S[q * SP + k] = acc;
    }
    __syncthreads();
    // masked max-subtracted softmax: one wave per live row, one key per lane (T <= 64), the shuffle tree
    for (int q = wave; q < L; q += SA_WAVES) {
        const float v = lane < L ? S[q * SP + lane] : -INFINITY;
        const float m = wave_max(v);
        const float e = lane < L ? expf(v - m) : 0.f;
        const float z = wave_sum(e);
        if (lane < L) S[q * SP + lane] = e / z;
    }
    __syncthreads();
    float* Pb = P + (int64_t)blockIdx.x * T * T;
    if (DROP) {
        const uint64_t ds = sa_drop_stream(dw, salt);
        const uint64_t e0 = ((uint64_t)dw.clip0 * heads + blockIdx.x) * (uint64_t)(T * T);
        const float inv = __fdiv_rn(1.0f, keep);
        for (int idx = tid; idx < T * T; idx += SA_THREADS) {
            const int q = idx / T, k = idx - q * T;
            const bool live = q < L && k < L;
            const float p = live ? S[q * SP + k] : 0.f;
            Pb[idx] = p;
            if (live) S[q * SP + k] = sa_drop_kept(ds, e0 + idx, keep) ? __fmul_rn(p, inv) : 0.f;
        }
        __syncthreads();
    } else {
        for (int idx = tid; idx < T * T; idx += SA_THREADS) {
            const int q = idx / T, k = idx - q * T;
            Pb[idx] = (q < L && k < L) ? S[q * SP + k] : 0.f;
        }
    }
    // ctx = P V: a thread per (q, d), lanes over d, k ascending
    for (int idx = tid; idx < T * dh; idx += SA_THREADS) {
        const int q = idx / dh, d = idx - q * dh;
        float acc = 0.f;
        if (q < L) {
            const float* sr = S + q * SP;
            for (int k = 0; k < L; ++k) acc = __fmaf_rn(sr[k], V[k * dhp + d], acc);
        }
        ctx[(row0 + q) * H + h * dh + d] = acc;
    }
}

// DROP (vl_mhsa_drop_bwd): the mask is drawn again from the counters.  The thread that stages element (q, k) of P leaves the DROPPED
// weight P M / keep in Ps (what dV needs) and the factor M / keep in the dS tile, where the same thread multiplies it into dP; the
// softmax's backward then reads the undropped P of its row from global memory.  No mask buffer, no second P, the same LDS.
template <bool DROP>
__global__ __launch_bounds__(SA_THREADS) void mhsa_bwd_kernel(const float* __restrict__ dctx, const float* __restrict__ qkv,
                                                              const float* __restrict__ P, const int32_t* __restrict__ seq_len,
                                                              float* __restrict__ dqkv, float* __restrict__ dposp, int T, int H,
                                                              int heads, int dh, float scale, float keep, uint32_t salt, SaDraw dw) {
    extern __shared__ __attribute__((aligned(16))) float sa_lds[];
    const int b = blockIdx.x / heads, h = blockIdx.x - b * heads;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int L = sa_len(seq_len, b, T), dhp = dh | 1, SP = T + 1;
    // two tiles used twice: (dO, V) for dP and dV, then (Q, K) for dK and dQ
    float* A = sa_lds;
    float* B = A + T * dhp;
    float* Ps = B + T * dhp;
    float* dS = Ps + T * SP;
    const int64_t row0 = (int64_t)b * T;
    sa_stage(A, dctx, row0, H, h * dh, L, dh, dhp, tid);
    sa_stage(B, qkv, row0, 3 * H, 2 * H + h * dh, L, dh, dhp, tid);
    const float* Pb = P + (int64_t)blockIdx.x * T * T;
    if (DROP) {
        const uint64_t ds = sa_drop_stream(dw, salt);
        const uint64_t e0 = ((uint64_t)dw.clip0 * heads + blockIdx.x) * (uint64_t)(T * T);
        const float inv = __fdiv_rn(1.0f, keep);
        for (int idx = tid; idx < L * L; idx += SA_THREADS) {
            const int q = idx / L, k = idx - q * L;
            const float f = sa_drop_kept(ds, e0 + (uint64_t)(q * T + k), keep) ? inv : 0.f;
            Ps[q * SP + k] = __fmul_rn(Pb[q * T + k], f);
            dS[q * SP + k] = f;
        }
    } else {
        for (int idx = tid; idx < L * L; idx += SA_THREADS) {
            const int q = idx / L, k = idx - q * L;
            Ps[q * SP + k] = Pb[q * T + k];
        }
    }
    __syncthreads();
    // dP = dO V^T: a thread per live (q, k), lanes over k
    for (int idx = tid; idx < L * L; idx += SA_THREADS) {
        const int q = idx / L, k = idx - q * L;
        const float* ar = A + q * dhp;
        const float* vr = B + k * dhp;
        float acc = 0.f;
        for (int d = 0; d < dh; ++d) acc = __fmaf_rn(ar[d], vr[d], acc);
        dS[q * SP + k] = DROP ? __fmul_rn(acc, dS[q * SP + k]) : acc;      // (the factor this thread left there)
    }
    // dV = P^T dO: a thread per (k, d), q ascending; dead rows zero
    float* dq = dqkv + row0 * 3 * H + h * dh;
    for (int idx = tid; idx < T * dh; idx += SA_THREADS) {
        const int k = idx / dh, d = idx - k * dh;
        float acc = 0.f;
        if (k < L)
            for (int q = 0; q < L; ++q) acc = __fmaf_rn(Ps[q * SP + k], A[q * dhp + d], acc);
        dq[(int64_t)k * 3 * H + 2 * H + d] = acc;
    }
    __syncthreads();
    // dS = P o (dP - rowsum(dP o P)): one wave per live row, in place
    for (int q = wave; q < L; q += SA_WAVES) {
        const float p = lane < L ? (DROP ? Pb[q * T + lane] : Ps[q * SP + lane]) : 0.f;
        const float g = lane < L ? dS[q * SP + lane] : 0.f;
        const float r = wave_sum(p * g);
        if (lane < L) dS[q * SP + lane] = p * (g - r);
    }
    __syncthreads();                                        // (every thread is past dV as well: the two tiles are free)
    sa_stage(A, qkv, row0, 3 * H, h * dh, L, dh, dhp, tid);          // Q
    sa_stage(B, qkv, row0, 3 * H, H + h * dh, L, dh, dhp, tid);      // K
    __syncthreads();
    for (int idx = tid; idx < T * dh; idx += SA_THREADS) {
        const int t = idx / dh, d = idx - t * dh;
        float aq = 0.f, ak = 0.f;
        if (t < L) {
            for (int k = 0; k < L; ++k) aq = __fmaf_rn(dS[t * SP + k], B[k * dhp + d], aq);       // dQ = dS K
            for (int q = 0; q < L; ++q) ak = __fmaf_rn(dS[q * SP + t], A[q * dhp + d], ak);       // dK = dS^T Q
        }
        dq[(int64_t)t * 3 * H + d] = aq * scale;
        dq[(int64_t)t * 3 * H + H + d] = ak * scale;
    }
    // per-clip partials of the position bias: diagonal r = k - q + T - 1, q ascending
    if (dposp) {
        for (int r = tid; r < 2 * T - 1; r += SA_THREADS) {
            float acc = 0.f;
            for (int q = 0; q < L; ++q) {
                const int k = q + r - (T - 1);
                if (k >= 0 && k < L) acc += dS[q * SP + k];
            }
            dposp[(int64_t)blockIdx.x * (2 * T - 1) + r] = acc;
        }
    }
}

// y = x in the live rows, 0 in the dead ones (x [batch T][W]); a grid-stride walk
__global__ __launch_bounds__(256) void live_rows_kernel(const float* __restrict__ x, const int32_t* __restrict__ seq_len,
                                                        float* __restrict__ y, int batch, int T, int W) {
    const int64_t total = (int64_t)batch * T * W, step = (int64_t)gridDim.x * 256;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += step) {
        const int64_t row = i / W;
        const int b = (int)(row / T), t = (int)(row - (int64_t)b * T);
        y[i] = t < sa_len(seq_len, b, T) ? x[i] : 0.f;
    }
}

static int sa_check(const char* who, int batch, int T, int H, int heads) {
    VL_CHECK(batch > 0 && T > 0 && H > 0 && heads > 0, "%s: batch %d, T %d, H %d, heads %d must be positive", who, batch, T, H, heads);
    VL_CHECK(T <= SA_MAX_T, "%s: T %d exceeds %d (a head's score tile lives in LDS, a key per lane)", who, T, SA_MAX_T);
    VL_CHECK(H <= SA_MAX_H, "%s: H %d exceeds %d", who, H, SA_MAX_H);
    VL_CHECK(H % heads == 0, "%s: heads %d does not divide H %d", who, heads, H);
    VL_CHECK(H / heads >= SA_MIN_DH && H / heads <= SA_MAX_DH, "%s: the head width H / heads = %d must lie in %d..%d", who, H / heads,
             SA_MIN_DH, SA_MAX_DH);
    VL_CHECK((int64_t)batch * heads < (1ll << 31), "%s: batch %d x heads %d workgroups exceed the grid", who, batch, heads);
    return 0;
}

// the two kernels may ask for more than the 64 KB a kernel gets by default: raised once per process to what the limits need
static int sa_raise_lds() {
    static bool done = false;
    if (!done) {
        VL_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(mhsa_fwd_kernel<false>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                   (int)sa_fwd_lds(SA_MAX_T, SA_MAX_DH)));
        VL_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(mhsa_bwd_kernel<false>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                   (int)sa_bwd_lds(SA_MAX_T, SA_MAX_DH)));
        VL_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(mhsa_fwd_kernel<true>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                   (int)sa_fwd_lds(SA_MAX_T, SA_MAX_DH)));
        VL_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(mhsa_bwd_kernel<true>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                   (int)sa_bwd_lds(SA_MAX_T, SA_MAX_DH)));
        done = true;
    }
    return 0;
}

extern "C" int vl_mhsa_fwd(const float* qkv, const float* pos, const int32_t* seq_len, float* P, float* ctx, int batch, int T, int H,
                           int heads, vl_stream_t stream) {
    VL_CHECK(qkv && P && ctx, "vl_mhsa_fwd: null pointer");
    if (int rc = sa_check("vl_mhsa_fwd", batch, T, H, heads)) return rc;
    if (int rc = sa_raise_lds()) return rc;
    const int dh = H / heads;
    hipLaunchKernelGGL(mhsa_fwd_kernel<false>, dim3(batch * heads), dim3(SA_THREADS), sa_fwd_lds(T, dh), (hipStream_t)stream, qkv, pos,
                       seq_len, P, ctx, T, H, heads, dh, 1.0f / sqrtf((float)dh), 1.0f, 0u, SaDraw{0, nullptr, 0});
    VL_LAUNCH_CHECK();
    return 0;
}

extern "C" int vl_mhsa_bwd(const float* dctx, const float* qkv, const float* P, const int32_t* seq_len, float* dqkv, float* dposp,
                           int batch, int T, int H, int heads, vl_stream_t stream) {
    VL_CHECK(dctx && qkv && P && dqkv, "vl_mhsa_bwd: null pointer");
    if (int rc = sa_check("vl_mhsa_bwd", batch, T, H, heads)) return rc;
    if (int rc = sa_raise_lds()) return rc;
    const int dh = H / heads;
    hipLaunchKernelGGL(mhsa_bwd_kernel<false>, dim3(batch * heads), dim3(SA_THREADS), sa_bwd_lds(T, dh), (hipStream_t)stream, dctx, qkv, P,
                       seq_len, dqkv, dposp, T, H, heads, dh, 1.0f / sqrtf((float)dh), 1.0f, 0u, SaDraw{0, nullptr, 0});
    VL_LAUNCH_CHECK();
    return 0;
}

// ---- the drop forms: the same launch shape and LDS, the seed given or formed from the step state when the kernel runs ----
static int sa_drop_check(const char* who, float keep, int64_t clip0, int batch) {
    VL_CHECK(sa_keep_ok(keep), "%s: keep %g must lie in (0, 1]", who, (double)keep);
    VL_CHECK(clip0 >= 0 && clip0 < (1ll << 31) - batch, "%s: clip0 %lld must lie in 0 .. 2^31 - batch", who, (long long)clip0);
    return 0;
}

static int mhsa_drop_fwd_run(const char* who, const float* qkv, const float* pos, const int32_t* seq_len, float* P, float* ctx, int batch,
                             int T, int H, int heads, float keep, uint32_t salt, SaDraw dw, hipStream_t stream) {
    VL_CHECK(qkv && P && ctx, "%s: null pointer", who);
    if (int rc = sa_check(who, batch, T, H, heads)) return rc;
    if (int rc = sa_drop_check(who, keep, dw.clip0, batch)) return rc;
    if (int rc = sa_raise_lds()) return rc;
    const int dh = H / heads;
    hipLaunchKernelGGL(mhsa_fwd_kernel<true>, dim3(batch * heads), dim3(SA_THREADS), sa_fwd_lds(T, dh), stream, qkv, pos, seq_len, P, ctx,
                       T, H, heads, dh, 1.0f / sqrtf((float)dh), keep, salt, dw);
    VL_LAUNCH_CHECK();
    return 0;
}

static int mhsa_drop_bwd_run(const char* who, const float* dctx, const float* qkv, const float* P, const int32_t* seq_len, float* dqkv,
                             float* dposp, int batch, int T, int H, int heads, float keep, uint32_t salt, SaDraw dw, hipStream_t stream) {
    VL_CHECK(dctx && qkv && P && dqkv, "%s: null pointer", who);
    if (int rc = sa_check(who, batch, T, H, heads)) return rc;
    if (int rc = sa_drop_check(who, keep, dw.clip0, batch)) return rc;
    if (int rc = sa_raise_lds()) return rc;
    const int dh = H / heads;
    hipLaunchKernelGGL(mhsa_bwd_kernel<true>, dim3(batch * heads), dim3(SA_THREADS), sa_bwd_lds(T, dh), stream, dctx, qkv, P, seq_len,
                       dqkv, dposp, T, H, heads, dh, 1.0f / sqrtf((float)dh), keep, salt, dw);
    VL_LAUNCH_CHECK();
    return 0;
}

extern "C" int vl_mhsa_drop_fwd(const float* qkv, const float* pos, const int32_t* seq_len, float* P, float* ctx, int batch, int T, int H,
                                int heads, float keep, uint64_t seed, uint32_t salt, int64_t clip0, vl_stream_t stream) {
    return mhsa_drop_fwd_run("vl_mhsa_drop_fwd", qkv, pos, seq_len, P, ctx, batch, T, H, heads, keep, salt, SaDraw{seed, nullptr, clip0},
                             (hipStream_t)stream);
}

extern "C" int vl_mhsa_drop_fwd_st(const float* qkv, const float* pos, const int32_t* seq_len, float* P, float* ctx, int batch, int T,
                                   int H, int heads, float keep, const vl_step_state* state, uint32_t salt, int64_t clip0,
                                   vl_stream_t stream) {
    VL_CHECK(state, "vl_mhsa_drop_fwd_st: null pointer");
    return mhsa_drop_fwd_run("vl_mhsa_drop_fwd_st", qkv, pos, seq_len, P, ctx, batch, T, H, heads, keep, salt, SaDraw{0, state, clip0},
                             (hipStream_t)stream);
}

extern "C" int vl_mhsa_drop_bwd(const float* dctx, const float* qkv, const float* P, const int32_t* seq_len, float* dqkv, float* dposp,
                                int batch, int T, int H, int heads, float keep, uint64_t seed, uint32_t salt, int64_t clip0,
                                vl_stream_t stream) {
    return mhsa_drop_bwd_run("vl_mhsa_drop_bwd", dctx, qkv, P, seq_len, dqkv, dposp, batch, T, H, heads, keep, salt,
                             SaDraw{seed, nullptr, clip0}, (hipStream_t)stream);
}

extern "C" int vl_mhsa_drop_bwd_st(const float* dctx, const float* qkv, const float* P, const int32_t* seq_len, float* dqkv, float* dposp,
                                   int batch, int T, int H, int heads, float keep, const vl_step_state* state, uint32_t salt,
                                   int64_t clip0, vl_stream_t stream) {
    VL_CHECK(state, "vl_mhsa_drop_bwd_st: null pointer");
    return mhsa_drop_bwd_run("vl_mhsa_drop_bwd_st", dctx, qkv, P, seq_len, dqkv, dposp, batch, T, H, heads, keep, salt,
                             SaDraw{0, state, clip0}, (hipStream_t)stream);
}

extern "C" int vl_live_rows(const float* x, const int32_t* seq_len, float* y, int batch, int T, int W, vl_stream_t stream) {
    VL_CHECK(x && seq_len && y, "vl_live_rows: null pointer");
    VL_CHECK(batch > 0 && T > 0 && W > 0, "vl_live_rows: batch %d, T %d, W %d must be positive", batch, T, W);
    const int64_t total = (int64_t)batch * T * W;
    const int blocks = (int)((total + 255) / 256 < 4096 ? (total + 255) / 256 : 4096);
    hipLaunchKernelGGL(live_rows_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, x, seq_len, y, batch, T, W);
    VL_LAUNCH_CHECK();
    return 0;
}
