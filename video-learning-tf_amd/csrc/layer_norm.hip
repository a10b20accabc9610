// Layer norm with a fused residual add, its backward, and the exact GELU (the encoder block of rnn_cell mhsa: sa_block encoder;
// vltf.h).  No atomics, every sum in one fixed order: what a launch writes for a clip is a function of that clip's inputs
// alone, so a clip's bits are the same alone or in any batch.  With L = min(max(seq_len[b], 0), T) live steps (NULL: T), rows t >= L of
// every input are never read; dead rows of y, sum, stats and dx are zeros.
//
// A ROW IN REGISTERS.  One wave per row, the row's W <= 1024 values in at most 16 registers per lane.  Which lane holds which element
// depends on W alone, never on a pointer: W % 4 == 0 -> lane holds the four-element granules lane, lane + 64, lane + 128, lane + 192
// (read and written 16 bytes at a time where every pointer of the launch is 16-byte aligned, and as four dwords where one is not: the
// same values in the same registers, so the same bits); else -> elements lane, lane + 64, ... one dword at a time.  A lane adds its
// registers in ascending index, then the xor butterfly of common.h adds the 64 lanes: one fixed tree.
// The mean comes first, then the variance of the centred values, both over registers: E[x^2] - mean^2 would lose the variance of a row
// whose mean is large against its spread (features of scale 40 at an offset of 40).
//
// Forward: 256 threads = four rows per workgroup, no LDS, no barrier.
// Backward: one workgroup of four waves per CLIP, because gamma's and beta's gradients are sums over the rows: the waves take four
// rows at a time (row 4g + wave), each leaves its row's dy x^ and dy in LDS [4][2W] (32 KB at W = 1024, static), and after a barrier
// thread tid adds the (at most four) rows IN ASCENDING t into the columns tid, tid + 256, ... of the 2W it owns (eight registers):
// dgb_partial [clips][2W] is the clip's sum over its live rows t = 0, 1, 2, ... in that order, whatever the wave count.
#include "common.h"

#define LN_THREADS 256
#define LN_WAVES (LN_THREADS / 64)
#define LN_MIN_W 8
#define LN_MAX_W 1024
#define LN_REGS (LN_MAX_W / 64)
#define LN_COLS ((2 * LN_MAX_W) / LN_THREADS)

__device__ __forceinline__ int ln_len(const int32_t* __restrict__ seq_len, int b, int T) {
    return seq_len ? min(max(seq_len[b], 0), T) : T;
}

// element index of register i of this lane (the layout above); >= W: the register is not part of the row
template <bool V4>
__device__ __forceinline__ int ln_elem(int i, int lane) {
    return V4 ? 4 * (lane + 64 * (i >> 2)) + (i & 3) : lane + 64 * i;
}

template <bool V4>
__device__ __forceinline__ void ln_load(float (&v)[LN_REGS], const float* __restrict__ p, int W, int lane, bool al16) {
    if (V4) {
#pragma unroll
        for (int j = 0; j < LN_REGS / 4; ++j) {
            const int e = 4 * (lane + 64 * j);
            if (e < W) {
                if (al16) {
                    const float4 q = *reinterpret_cast<const float4*>(p + e);
                    v[4 * j] = q.x, v[4 * j + 1] = q.y, v[4 * j + 2] = q.z, v[4 * j + 3] = q.w;
                } else {
                    v[4 * j] = p[e], v[4 * j + 1] = p[e + 1], v[4 * j + 2] = p[e + 2], v[4 * j + 3] = p[e + 3];
                }
            } else {
                v[4 * j] = v[4 * j + 1] = v[4 * j + 2] = v[4 * j + 3] = 0.f;
            }
        }
    } else {
#pragma unroll
        for (int i = 0; i < LN_REGS; ++i) {
            const int e = lane + 64 * i;
            v[i] = e < W ? p[e] : 0.f;
        }
    }
}

template <bool V4>
__device__ __forceinline__ void ln_store(const float (&v)[LN_REGS], float* __restrict__ p, int W, int lane, bool al16) {
    if (V4) {
#pragma unroll
        for (int j = 0; j < LN_REGS / 4; ++j) {
            const int e = 4 * (lane + 64 * j);
            if (e < W) {
                if (al16) {
                    *reinterpret_cast<float4*>(p + e) = make_float4(v[4 * j], v[4 * j + 1], v[4 * j + 2], v[4 * j + 3]);
                } else {
                    p[e] = v[4 * j], p[e + 1] = v[4 * j + 1], p[e + 2] = v[4 * j + 2], p[e + 3] = v[4 * j + 3];
                }
            }
        }
    } else {
#pragma unroll
        for (int i = 0; i < LN_REGS; ++i) {
            const int e = lane + 64 * i;
            if (e < W) p[e] = v[i];
        }
    }
}

// the sum over the row of v (registers past W hold 0): the lane's registers ascending, then the butterfly
__device__ __forceinline__ float ln_row_sum(const float (&v)[LN_REGS]) {
    float a = 0.f;
#pragma unroll
    for (int i = 0; i < LN_REGS; ++i) a = __fadd_rn(a, v[i]);
    return wave_sum(a);
}

// what the drop forms draw with: the branch's element keep and path keep (either may be 1: that option draws nothing), the
// salts of the element and path streams, which of the layer's two branches this is, and seed / step state / clip0 (common.h: SaDraw)
struct LnDrop {
    float keep, keep_path;
    uint32_t salt_elem, salt_path;
    int branch;
    SaDraw dw;
};

// DROP (vl_add_layer_norm_drop_fwd): s = x + r f with the branch factor f of common.h, drawn in registers between the load of r and
// the add; the element's counter is ((clip0 + b) T + t) W + col, the path's 2 (clip0 + b) + branch.  Everything else is the kernel
// as it was, and without DROP it is that kernel instruction for instruction.
template <bool V4, bool DROP>
__global__ __launch_bounds__(LN_THREADS) void add_layer_norm_fwd_kernel(const float* __restrict__ x, const float* __restrict__ r,
                                                                        float* __restrict__ sum, float* __restrict__ y,
                                                                        const float* __restrict__ gamma, const float* __restrict__ beta,
                                                                        float* __restrict__ stats, const int32_t* __restrict__ seq_len,
                                                                        int64_t rows, int T, int W, float eps, bool al16, LnDrop dp) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t row = (int64_t)blockIdx.x * LN_WAVES + wave;
    if (row >= rows) return;                                  // (no barrier in this kernel)
    const int64_t off = row * W;
    float s[LN_REGS];
    bool dead = false;
    if (seq_len) {                                            // (rows < 2^31: a 32-bit division, and none without lengths)
        const uint32_t b = (uint32_t)row / (uint32_t)T, t = (uint32_t)row - b * (uint32_t)T;
        dead = (int)t >= ln_len(seq_len, (int)b, T);
    }
    if (dead) {                                               // a dead row: zeros, nothing read
#pragma unroll
        for (int i = 0; i < LN_REGS; ++i) s[i] = 0.f;
        ln_store<V4>(s, y + off, W, lane, al16);
        if (sum) ln_store<V4>(s, sum + off, W, lane, al16);
        if (lane < 2) stats[2 * row + lane] = 0.f;
        return;
    }
    float g[LN_REGS], bt[LN_REGS];                            // every load of the row's chain issued before the first reduction
    ln_load<V4>(s, x + off, W, lane, al16);
    ln_load<V4>(g, gamma, W, lane, al16);
    ln_load<V4>(bt, beta, W, lane, al16);
    if (r) {
        float q[LN_REGS];
        ln_load<V4>(q, r + off, W, lane, al16);
        if (DROP) {
            const uint64_t clip = (uint64_t)dp.dw.clip0 + (uint32_t)row / (uint32_t)T;
            const float fp = sa_path_factor(sa_drop_stream(dp.dw, dp.salt_path), 2 * clip + (uint64_t)dp.branch, dp.keep_path);
            const uint64_t se = sa_drop_stream(dp.dw, dp.salt_elem);
            const uint64_t e0 = ((uint64_t)dp.dw.clip0 * (uint64_t)T + (uint64_t)row) * (uint64_t)W;
            const float inv = __fdiv_rn(1.0f, dp.keep);
#pragma unroll
            for (int i = 0; i < LN_REGS; ++i) {
                const int e = ln_elem<V4>(i, lane);
                if (e < W) s[i] = sa_branch_add(s[i], q[i], sa_branch_factor(se, e0 + (uint64_t)e, dp.keep, inv, fp));
            }
        } else {
#pragma unroll
            for (int i = 0; i < LN_REGS; ++i) s[i] = __fadd_rn(s[i], q[i]);
        }
    }
    if (sum) ln_store<V4>(s, sum + off, W, lane, al16);
    const float w = (float)W;                                 // (a division, not a reciprocal: a row of one value has exactly that mean)
    const float mean = __fdiv_rn(ln_row_sum(s), w);
    float c[LN_REGS];
#pragma unroll
    for (int i = 0; i < LN_REGS; ++i) c[i] = ln_elem<V4>(i, lane) < W ? __fsub_rn(s[i], mean) : 0.f;
    float sq[LN_REGS];
#pragma unroll
    for (int i = 0; i < LN_REGS; ++i) sq[i] = __fmul_rn(c[i], c[i]);
    const float var = __fdiv_rn(ln_row_sum(sq), w);
    const float rstd = 1.0f / sqrtf(var + eps);
#pragma unroll
    for (int i = 0; i < LN_REGS; ++i) c[i] = __fmaf_rn(__fmul_rn(c[i], rstd), g[i], bt[i]);
    ln_store<V4>(c, y + off, W, lane, al16);
    if (lane == 0) {
        stats[2 * row] = mean;
        stats[2 * row + 1] = rstd;
    }
}

template <bool V4>
__global__ __launch_bounds__(LN_THREADS) void layer_norm_bwd_kernel(const float* __restrict__ dy, const float* __restrict__ s,
                                                                    const float* __restrict__ gamma, const float* __restrict__ stats,
                                                                    const float* __restrict__ dres, float* __restrict__ dx,
                                                                    float* __restrict__ dgbp, const int32_t* __restrict__ seq_len, int T,
                                                                    int W, bool al16) {
    __shared__ __attribute__((aligned(16))) float part[LN_WAVES][2 * LN_MAX_W];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int b = blockIdx.x;
    const int L = ln_len(seq_len, b, T);                      // uniform over the workgroup: every wave runs the same groups
    const float fw = (float)W;
    float g[LN_REGS];
    ln_load<V4>(g, gamma, W, lane, al16);
    float acc[LN_COLS];
#pragma unroll
    for (int k = 0; k < LN_COLS; ++k) acc[k] = 0.f;
    for (int t0 = 0; t0 < L; t0 += LN_WAVES) {
        const int t = t0 + wave;
        if (t < L) {
            const int64_t row = (int64_t)b * T + t, off = row * W;
            const float mean = stats[2 * row], rstd = stats[2 * row + 1];
            float d[LN_REGS], xh[LN_REGS], w[LN_REGS];
            ln_load<V4>(d, dy + off, W, lane, al16);
            ln_load<V4>(xh, s + off, W, lane, al16);
#pragma unroll
            for (int i = 0; i < LN_REGS; ++i) {
                const int e = ln_elem<V4>(i, lane);
                xh[i] = e < W ? __fmul_rn(__fsub_rn(xh[i], mean), rstd) : 0.f;
                w[i] = __fmul_rn(d[i], xh[i]);                // dy x^: gamma's share of this row
                if (e < W) {
                    part[wave][e] = w[i];
                    part[wave][W + e] = d[i];
                }
                d[i] = __fmul_rn(d[i], g[i]);                 // dy^ = dy gamma
                w[i] = __fmul_rn(d[i], xh[i]);
            }
            const float m1 = __fdiv_rn(ln_row_sum(d), fw);    // mean(dy^)
            const float m2 = __fdiv_rn(ln_row_sum(w), fw);    // mean(dy^ x^)
#pragma unroll
            for (int i = 0; i < LN_REGS; ++i) d[i] = __fmul_rn(rstd, __fsub_rn(__fsub_rn(d[i], m1), __fmul_rn(xh[i], m2)));
            if (dres) {
                ln_load<V4>(w, dres + off, W, lane, al16);
#pragma unroll
                for (int i = 0; i < LN_REGS; ++i) d[i] = __fadd_rn(d[i], w[i]);
            }
            ln_store<V4>(d, dx + off, W, lane, al16);
        }
        __syncthreads();
        const int live = min(LN_WAVES, L - t0);
#pragma unroll
        for (int k = 0; k < LN_COLS; ++k) {
            const int c = tid + LN_THREADS * k;
            if (c < 2 * W)
                for (int j = 0; j < live; ++j) acc[k] = __fadd_rn(acc[k], part[j][c]);
        }
        __syncthreads();
    }
#pragma unroll
    for (int k = 0; k < LN_COLS; ++k) {
        const int c = tid + LN_THREADS * k;
        if (c < 2 * W) dgbp[(int64_t)b * 2 * W + c] = acc[k];
    }
    float z[LN_REGS];
#pragma unroll
    for (int i = 0; i < LN_REGS; ++i) z[i] = 0.f;
    for (int t = L + wave; t < T; t += LN_WAVES) ln_store<V4>(z, dx + ((int64_t)b * T + t) * W, W, lane, al16);
}

// ---- GELU, the exact form: f = u Phi(u), Phi(u) = erfc(-u / sqrt 2) / 2 -----------------------------------------------------------------
// erfc keeps its relative accuracy where 1 + erf(u / sqrt 2) cancels (u < -3); past u = -14 it underflows to 0 and past u = 6 Phi is 1:
// f and du stay finite there, the gradient Phi + u phi(u) goes to 0 and 1 (exp(-u^2 / 2) underflows to 0 long before u phi could overflow).
__device__ __forceinline__ float gelu_phi_cdf(float u) { return 0.5f * erfcf(-0.70710678118654752440f * u); }
__device__ __forceinline__ float gelu_f(float u) { return u * gelu_phi_cdf(u); }
__device__ __forceinline__ float gelu_df(float u) {
    return __fmaf_rn(u, 0.39894228040143267794f * expf(-0.5f * u * u), gelu_phi_cdf(u));
}

// 16-byte accesses over the first count / 4 granules where both pointers are 16-byte aligned (n4 = 0 where not), a dword tail
__global__ __launch_bounds__(256) void gelu_fwd_kernel(const float* __restrict__ u, float* __restrict__ f, int64_t n4, int64_t count) {
    const int64_t step = (int64_t)gridDim.x * 256;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += step) {
        const float4 q = reinterpret_cast<const float4*>(u)[i];
        reinterpret_cast<float4*>(f)[i] = make_float4(gelu_f(q.x), gelu_f(q.y), gelu_f(q.z), gelu_f(q.w));
    }
    for (int64_t i = 4 * n4 + (int64_t)blockIdx.x * 256 + threadIdx.x; i < count; i += step) f[i] = gelu_f(u[i]);
}

// du may be df: an element is read before it is written, by the thread that writes it (no __restrict__ on the two)
__global__ __launch_bounds__(256) void gelu_bwd_kernel(const float* df, const float* __restrict__ u, float* du, int64_t n4, int64_t count) {
    const int64_t step = (int64_t)gridDim.x * 256;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += step) {
        const float4 q = reinterpret_cast<const float4*>(u)[i];
        const float4 d = reinterpret_cast<const float4*>(df)[i];
        reinterpret_cast<float4*>(du)[i] = make_float4(d.x * gelu_df(q.x), d.y * gelu_df(q.y), d.z * gelu_df(q.z), d.w * gelu_df(q.w));
    }
    for (int64_t i = 4 * n4 + (int64_t)blockIdx.x * 256 + threadIdx.x; i < count; i += step) du[i] = df[i] * gelu_df(u[i]);
}

static inline bool al16_of(const void* p) { return p == nullptr || ((uintptr_t)p & 15) == 0; }

static int ln_check(const char* who, int clips, int T, int W) {
    VL_CHECK(clips > 0 && T > 0, "%s: clips %d, T %d must be positive", who, clips, T);
    VL_CHECK(W >= LN_MIN_W && W <= LN_MAX_W, "%s: the row width W %d must lie in %d..%d (a row lives in one wave's registers)", who, W,
             LN_MIN_W, LN_MAX_W);
    VL_CHECK((int64_t)clips * T < (1ll << 31), "%s: clips %d x T %d rows exceed the grid", who, clips, T);
    return 0;
}

extern "C" int vl_add_layer_norm_fwd(const float* x, const float* r, float* sum, float* y, const float* gamma, const float* beta,
                                     float* stats, int clips, int T, int W, float eps, const int32_t* seq_len, vl_stream_t stream) {
    VL_CHECK(x && y && gamma && beta && stats, "vl_add_layer_norm_fwd: null pointer");
    if (int rc = ln_check("vl_add_layer_norm_fwd", clips, T, W)) return rc;
    VL_CHECK(eps > 0.f && eps - eps == 0.f, "vl_add_layer_norm_fwd: eps %g must be positive and finite", (double)eps);
    const int64_t rows = (int64_t)clips * T;
    const bool al = al16_of(x) && al16_of(r) && al16_of(sum) && al16_of(y) && al16_of(gamma) && al16_of(beta);
    const dim3 grid((unsigned)((rows + LN_WAVES - 1) / LN_WAVES));
    const LnDrop none = {1.f, 1.f, 0u, 0u, 0, {0, nullptr, 0}};
    if (W % 4 == 0)
        hipLaunchKernelGGL((add_layer_norm_fwd_kernel<true, false>), grid, dim3(LN_THREADS), 0, (hipStream_t)stream, x, r, sum, y, gamma,
                           beta, stats, seq_len, rows, T, W, eps, al, none);
    else
        hipLaunchKernelGGL((add_layer_norm_fwd_kernel<false, false>), grid, dim3(LN_THREADS), 0, (hipStream_t)stream, x, r, sum, y, gamma,
                           beta, stats, seq_len, rows, T, W, eps, false, none);
    VL_LAUNCH_CHECK();
    return 0;
}

// ---- the drop forms ----------------------------------------------------------------------------------------------------
static int ln_drop_check(const char* who, const LnDrop& dp, int clips) {
    VL_CHECK(sa_keep_ok(dp.keep), "%s: keep %g must lie in (0, 1]", who, (double)dp.keep);
    VL_CHECK(sa_keep_ok(dp.keep_path), "%s: keep_path %g must lie in (0, 1]", who, (double)dp.keep_path);
    VL_CHECK(dp.branch == 0 || dp.branch == 1, "%s: branch %d must be 0 (attention) or 1 (feed-forward)", who, dp.branch);
    VL_CHECK(dp.dw.clip0 >= 0 && dp.dw.clip0 < (1ll << 31) - clips, "%s: clip0 %lld must lie in 0 .. 2^31 - clips", who,
             (long long)dp.dw.clip0);
    return 0;
}

static int add_layer_norm_drop_run(const char* who, const float* x, const float* r, float* sum, float* y, const float* gamma,
                                   const float* beta, float* stats, int clips, int T, int W, float eps, const int32_t* seq_len, LnDrop dp,
                                   hipStream_t stream) {
    VL_CHECK(x && r && y && gamma && beta && stats, "%s: null pointer", who);
    if (int rc = ln_check(who, clips, T, W)) return rc;
    VL_CHECK(eps > 0.f && eps - eps == 0.f, "%s: eps %g must be positive and finite", who, (double)eps);
    if (int rc = ln_drop_check(who, dp, clips)) return rc;
    const int64_t rows = (int64_t)clips * T;
    const bool al = al16_of(x) && al16_of(r) && al16_of(sum) && al16_of(y) && al16_of(gamma) && al16_of(beta);
    const dim3 grid((unsigned)((rows + LN_WAVES - 1) / LN_WAVES));
    if (W % 4 == 0)
        hipLaunchKernelGGL((add_layer_norm_fwd_kernel<true, true>), grid, dim3(LN_THREADS), 0, stream, x, r, sum, y, gamma, beta, stats,
                           seq_len, rows, T, W, eps, al, dp);
    else
        hipLaunchKernelGGL((add_layer_norm_fwd_kernel<false, true>), grid, dim3(LN_THREADS), 0, stream, x, r, sum, y, gamma, beta, stats,
                           seq_len, rows, T, W, eps, false, dp);
    VL_LAUNCH_CHECK();
    return 0;
}

extern "C" int vl_add_layer_norm_drop_fwd(const float* x, const float* r, float* sum, float* y, const float* gamma, const float* beta,
                                          float* stats, int clips, int T, int W, float eps, const int32_t* seq_len, float keep,
                                          float keep_path, uint64_t seed, uint32_t salt_elem, uint32_t salt_path, int branch, int64_t clip0,
                                          vl_stream_t stream) {
    return add_layer_norm_drop_run("vl_add_layer_norm_drop_fwd", x, r, sum, y, gamma, beta, stats, clips, T, W, eps, seq_len,
                                   LnDrop{keep, keep_path, salt_elem, salt_path, branch, {seed, nullptr, clip0}}, (hipStream_t)stream);
}

extern "C" int vl_add_layer_norm_drop_fwd_st(const float* x, const float* r, float* sum, float* y, const float* gamma, const float* beta,
                                             float* stats, int clips, int T, int W, float eps, const int32_t* seq_len, float keep,
                                             float keep_path, const vl_step_state* state, uint32_t salt_elem, uint32_t salt_path,
                                             int branch, int64_t clip0, vl_stream_t stream) {
    VL_CHECK(state, "vl_add_layer_norm_drop_fwd_st: null pointer");
    return add_layer_norm_drop_run("vl_add_layer_norm_drop_fwd_st", x, r, sum, y, gamma, beta, stats, clips, T, W, eps, seq_len,
                                   LnDrop{keep, keep_path, salt_elem, salt_path, branch, {0, state, clip0}}, (hipStream_t)stream);
}

// dr = ds f over rows [clips T][W], zeros in the dead rows (ds never read there): the gradient that enters a branch the forward
// dropped, f drawn again from the same counters.  The counter of flat element i is clip0 T W + i, so the draw is a function of the
// element alone: the 16-byte interior (n4 granules where both pointers allow it) and the dword tail give the same bits.
__device__ __forceinline__ float branch_drop_grad_elem(const float* __restrict__ ds, int64_t i, const int32_t* __restrict__ seq_len,
                                                       int T, int W, const LnDrop& dp, uint64_t se, uint64_t sp, float inv, float v,
                                                       bool have) {
#pragma clang fp contract(off)
    const int64_t row = i / W;
    const int b = (int)(row / T), t = (int)(row - (int64_t)b * T);
    if (t >= ln_len(seq_len, b, T)) return 0.f;
    const float fp = sa_path_factor(sp, 2 * ((uint64_t)dp.dw.clip0 + (uint64_t)b) + (uint64_t)dp.branch, dp.keep_path);
    const uint64_t e = (uint64_t)dp.dw.clip0 * (uint64_t)T * (uint64_t)W + (uint64_t)i;
    const float d = have ? v : ds[i];
    return d * sa_branch_factor(se, e, dp.keep, inv, fp);
}

__global__ __launch_bounds__(256) void branch_drop_grad_kernel(const float* __restrict__ ds, float* __restrict__ dr,
                                                               const int32_t* __restrict__ seq_len, int T, int W, int64_t n4,
                                                               int64_t count, LnDrop dp) {
    const int64_t step = (int64_t)gridDim.x * 256;
    const uint64_t se = sa_drop_stream(dp.dw, dp.salt_elem), sp = sa_drop_stream(dp.dw, dp.salt_path);
    const float inv = __fdiv_rn(1.0f, dp.keep);
    for (int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x; g < n4; g += step) {
        // (W >= 8: a granule lies in one row or two.  Both live: one 16-byte read; else its live elements alone are read)
        const int64_t i = 4 * g, row0 = i / W, row1 = (i + 3) / W;
        const int b0 = (int)(row0 / T), b1 = (int)(row1 / T);
        const bool live = (int)(row0 - (int64_t)b0 * T) < ln_len(seq_len, b0, T) && (int)(row1 - (int64_t)b1 * T) < ln_len(seq_len, b1, T);
        float4 q = make_float4(0.f, 0.f, 0.f, 0.f);
        if (live) q = reinterpret_cast<const float4*>(ds)[g];
        float4 o;
        o.x = branch_drop_grad_elem(ds, i, seq_len, T, W, dp, se, sp, inv, q.x, live);
        o.y = branch_drop_grad_elem(ds, i + 1, seq_len, T, W, dp, se, sp, inv, q.y, live);
        o.z = branch_drop_grad_elem(ds, i + 2, seq_len, T, W, dp, se, sp, inv, q.z, live);
        o.w = branch_drop_grad_elem(ds, i + 3, seq_len, T, W, dp, se, sp, inv, q.w, live);
        reinterpret_cast<float4*>(dr)[g] = o;
    }
    for (int64_t i = 4 * n4 + (int64_t)blockIdx.x * 256 + threadIdx.x; i < count; i += step)
        dr[i] = branch_drop_grad_elem(ds, i, seq_len, T, W, dp, se, sp, inv, 0.f, false);
}

static int branch_drop_grad_run(const char* who, const float* ds, float* dr, int clips, int T, int W, const int32_t* seq_len, LnDrop dp,
                                hipStream_t stream) {
    VL_CHECK(ds && dr, "%s: null pointer", who);
    if (int rc = ln_check(who, clips, T, W)) return rc;
    if (int rc = ln_drop_check(who, dp, clips)) return rc;
    const int64_t count = (int64_t)clips * T * W;
    const int64_t n4 = ((uintptr_t)ds & 15) == 0 && ((uintptr_t)dr & 15) == 0 ? count / 4 : 0;
    const int64_t work = (count + 3) / 4, blocks = (work + 255) / 256;
    hipLaunchKernelGGL(branch_drop_grad_kernel, dim3((unsigned)(blocks < 4096 ? blocks : 4096)), dim3(256), 0, stream, ds, dr, seq_len, T,
                       W, n4, count, dp);
    VL_LAUNCH_CHECK();
    return 0;
}

extern "C" int vl_branch_drop_grad(const float* ds, float* dr, int clips, int T, int W, const int32_t* seq_len, float keep,
                                   float keep_path, uint64_t seed, uint32_t salt_elem, uint32_t salt_path, int branch, int64_t clip0,
                                   vl_stream_t stream) {
    return branch_drop_grad_run("vl_branch_drop_grad", ds, dr, clips, T, W, seq_len,
                                LnDrop{keep, keep_path, salt_elem, salt_path, branch, {seed, nullptr, clip0}}, (hipStream_t)stream);
}

extern "C" int vl_branch_drop_grad_st(const float* ds, float* dr, int clips, int T, int W, const int32_t* seq_len, float keep,
                                      float keep_path, const vl_step_state* state, uint32_t salt_elem, uint32_t salt_path, int branch,
                                      int64_t clip0, vl_stream_t stream) {
    VL_CHECK(state, "vl_branch_drop_grad_st: null pointer");
    return branch_drop_grad_run("vl_branch_drop_grad_st", ds, dr, clips, T, W, seq_len,
                                LnDrop{keep, keep_path, salt_elem, salt_path, branch, {0, state, clip0}}, (hipStream_t)stream);
}

extern "C" int vl_layer_norm_bwd(const float* dy, const float* s, const float* gamma, const float* stats, const float* dres, float* dx,
                                 float* dgb_partial, int clips, int T, int W, const int32_t* seq_len, vl_stream_t stream) {
    VL_CHECK(dy && s && gamma && stats && dx && dgb_partial, "vl_layer_norm_bwd: null pointer");
    if (int rc = ln_check("vl_layer_norm_bwd", clips, T, W)) return rc;
    const bool al = al16_of(dy) && al16_of(s) && al16_of(gamma) && al16_of(dres) && al16_of(dx);
    if (W % 4 == 0)
        hipLaunchKernelGGL(layer_norm_bwd_kernel<true>, dim3(clips), dim3(LN_THREADS), 0, (hipStream_t)stream, dy, s, gamma, stats, dres, dx,
                           dgb_partial, seq_len, T, W, al);
    else
        hipLaunchKernelGGL(layer_norm_bwd_kernel<false>, dim3(clips), dim3(LN_THREADS), 0, (hipStream_t)stream, dy, s, gamma, stats, dres,
                           dx, dgb_partial, seq_len, T, W, false);
    VL_LAUNCH_CHECK();
    return 0;
}

static inline int gelu_blocks(int64_t count) {
    const int64_t work = (count + 3) / 4, blocks = (work + 255) / 256;
    return (int)(blocks < 4096 ? blocks : 4096);
}

extern "C" int vl_gelu_fwd(const float* u, float* f, int64_t count, vl_stream_t stream) {
    VL_CHECK(u && f, "vl_gelu_fwd: null pointer");
    VL_CHECK(count > 0, "vl_gelu_fwd: count %lld must be positive", (long long)count);
    const int64_t n4 = al16_of(u) && al16_of(f) ? count / 4 : 0;
    hipLaunchKernelGGL(gelu_fwd_kernel, dim3(gelu_blocks(count)), dim3(256), 0, (hipStream_t)stream, u, f, n4, count);
    VL_LAUNCH_CHECK();
    return 0;
}

extern "C" int vl_gelu_bwd(const float* df, const float* u, float* du, int64_t count, vl_stream_t stream) {
    VL_CHECK(df && u && du, "vl_gelu_bwd: null pointer");
    VL_CHECK(count > 0, "vl_gelu_bwd: count %lld must be positive", (long long)count);
    const int64_t n4 = al16_of(df) && al16_of(u) && al16_of(du) ? count / 4 : 0;
    hipLaunchKernelGGL(gelu_bwd_kernel, dim3(gelu_blocks(count)), dim3(256), 0, (hipStream_t)stream, df, u, du, n4, count);
    VL_LAUNCH_CHECK();
    return 0;
}
