// NetVLAD pooling over time (fusion `vlad`; vltf.h).
// One workgroup per clip (VLAD_THREADS forward, VLAD_BWD_THREADS backward), no atomics, every sum in one fixed order (t ascending, the shuffle tree of a wave, the
// waves in order): what a workgroup writes is a function of its clip's inputs alone, so a clip's bits are the same alone or in any
// batch.  With L = min(max(seq_len[b], 1), T) live steps (NULL: T), rows t >= L of h and s are never read.
//
// The intra-normalisation makes the clusters independent of each other in both directions (the whole-descriptor norm is the constant
// 1 / sqrt(K)); only the softmax over k couples them, per row.  So a wave does a row's softmax with a lane per cluster (K <= 64), and
// everything else runs per cluster: a thread per column j of h, VLAD_SLAB clusters (forward) or steps (backward) in registers at a
// time, the slab's assignments broadcast out of LDS.  The unnormalised V is staged in y, dV in dcp and da in ds -- the outputs that
// will hold them scaled -- and read back by the same workgroup behind a barrier: no LDS is spent on them (K HO is up to 64 KB).
#include "common.h"

#define VLAD_THREADS 256
#define VLAD_WAVES (VLAD_THREADS / 64)
#define VLAD_BWD_THREADS 1024    // the backward: 16 waves share a clip's (cluster, step) dot products, 4 groups of 256 its step slabs
#define VLAD_BWD_WAVES (VLAD_BWD_THREADS / 64)
#define VLAD_BWD_GROUPS (VLAD_BWD_THREADS / VLAD_THREADS)
#define VLAD_MAX_K 64
#define VLAD_MAX_HO 1024
#define VLAD_MAX_KHO 16384
#define VLAD_MAX_T 1024
#define VLAD_SLAB 8
#define VLAD_EPS 1e-12f          // tf.nn.l2_normalize's epsilon on |V_k|^2
#define VLAD_RMAX 1e6f           // rsqrt(VLAD_EPS): the scale of a cluster below the epsilon, stored exactly

__device__ __forceinline__ int vlad_len(const int32_t* __restrict__ seq_len, int b, int T) {
    return seq_len ? min(max(seq_len[b], 1), T) : T;
}

// a may alias s: element [t][k] is read, then written, by one lane
__global__ __launch_bounds__(VLAD_THREADS) void netvlad_fwd_kernel(const float* s, const float* __restrict__ c,
                                                                   const float* __restrict__ h, const int32_t* __restrict__ seq_len,
                                                                   float* a, float* __restrict__ r, float* y, int T, int HO, int K) {
    __shared__ __attribute__((aligned(16))) float as[VLAD_MAX_T * VLAD_SLAB];      // the slab's assignments [t][VLAD_SLAB]
    __shared__ float part[VLAD_WAVES][VLAD_SLAB];
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int L = vlad_len(seq_len, b, T);
    const float* sb = s + (int64_t)b * T * K;
    float* ab = a + (int64_t)b * T * K;
    // soft assignment: one wave per row, a lane per cluster
    for (int t = wave; t < T; t += VLAD_WAVES) {
        float w = 0.f;
        if (t < L) {
            const float v = lane < K ? sb[(int64_t)t * K + lane] : -INFINITY;
            const float mx = wave_max(v);
            const float e = lane < K ? expf(v - mx) : 0.f;
            w = e / wave_sum(e);
        }
        if (lane < K) ab[(int64_t)t * K + lane] = w;
    }
    __syncthreads();                                        // the clip's rows of a are read back below
    const float* hb = h + (int64_t)b * T * HO;
    float* yb = y + (int64_t)b * K * HO;
    const float isk = 1.f / sqrtf((float)K);
    for (int k0 = 0; k0 < K; k0 += VLAD_SLAB) {
        for (int idx = tid; idx < L * VLAD_SLAB; idx += VLAD_THREADS) {
            const int t = idx / VLAD_SLAB, kk = idx - t * VLAD_SLAB;
            as[idx] = k0 + kk < K ? ab[(int64_t)t * K + k0 + kk] : 0.f;
        }
        __syncthreads();
        float ss[VLAD_SLAB];
#pragma unroll
        for (int kk = 0; kk < VLAD_SLAB; ++kk) ss[kk] = 0.f;
        for (int col = tid; col < HO; col += VLAD_THREADS) {    // a thread per column, t ascending: coalesced rows of h
            float acc[VLAD_SLAB], m[VLAD_SLAB];
#pragma unroll
            for (int kk = 0; kk < VLAD_SLAB; ++kk) acc[kk] = m[kk] = 0.f;
            for (int t = 0; t < L; ++t) {
                const float hv = hb[(int64_t)t * HO + col];
#pragma unroll
                for (int kk = 0; kk < VLAD_SLAB; ++kk) {
                    const float w = as[t * VLAD_SLAB + kk];
                    acc[kk] = __fmaf_rn(w, hv, acc[kk]);
                    m[kk] += w;
                }
            }
#pragma unroll
            for (int kk = 0; kk < VLAD_SLAB; ++kk) {
                if (k0 + kk < K) {
                    const float v = acc[kk] - m[kk] * c[(int64_t)(k0 + kk) * HO + col];
                    yb[(int64_t)(k0 + kk) * HO + col] = v;                           // V, unnormalised: scaled below by this thread
                    ss[kk] = __fmaf_rn(v, v, ss[kk]);
                }
            }
        }
#pragma unroll
        for (int kk = 0; kk < VLAD_SLAB; ++kk) {
            const float v = wave_sum(ss[kk]);
            if (lane == 0) part[wave][kk] = v;
        }
        __syncthreads();
#pragma unroll
        for (int kk = 0; kk < VLAD_SLAB; ++kk) {
            if (k0 + kk < K) {
                float n2 = part[0][kk];
                for (int w = 1; w < VLAD_WAVES; ++w) n2 += part[w][kk];
                // (an n2 one or two ulps above the epsilon gives 1 / sqrtf(n2) = 1e6f after rounding, and the backward, which reads
                // r < 1e6 as "normalised", then skips the projection for it: the rule of vltf.h as written, at a cluster whose
                // gradient is at the rounding of either branch)
                const float rk = n2 > VLAD_EPS ? 1.f / sqrtf(n2) : VLAD_RMAX;
                if (tid == 0) r[(int64_t)b * K + k0 + kk] = rk;
                const float sc = rk * isk;
                for (int col = tid; col < HO; col += VLAD_THREADS) yb[(int64_t)(k0 + kk) * HO + col] *= sc;
            }
        }
        __syncthreads();                                    // as and part are rewritten by the next slab
    }
}

// What a thread count changes here is which wave or thread forms a value, never how: every output's bits are those of any other count.
__global__ __launch_bounds__(VLAD_BWD_THREADS) void netvlad_bwd_kernel(const float* __restrict__ dy, const float* __restrict__ h,
                                                                   const float* __restrict__ a, const float* __restrict__ r,
                                                                   const float* __restrict__ y, const float* __restrict__ c,
                                                                   const int32_t* __restrict__ seq_len, float* ds,
                                                                   float* __restrict__ dh, float* dcp, int T, int HO, int K) {
    __shared__ __attribute__((aligned(16))) float as[VLAD_BWD_GROUPS][VLAD_MAX_K * VLAD_SLAB];    // a group's step slab of a: [k][VLAD_SLAB]
    __shared__ float ms[VLAD_MAX_K];
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int L = vlad_len(seq_len, b, T);
    const float* hb = h + (int64_t)b * T * HO;
    const float* ab = a + (int64_t)b * T * K;
    const float* dyb = dy + (int64_t)b * K * HO;
    const float* yb = y + (int64_t)b * K * HO;
    float* dsb = ds + (int64_t)b * T * K;
    float* dvb = dcp + (int64_t)b * K * HO;                 // dV until the last loop scales it to the centres' partials
    const float sk = sqrtf((float)K), isk = 1.f / sk;
    constexpr int NJ = VLAD_MAX_HO / 64;
    // a wave per cluster -- TS waves where there are fewer clusters than waves, each with every TS-th step --: dV_k through the
    // normalisation, then da_tk = dV_k . (h_t - c_k) for its live steps, staged in ds
    const int TS = K < VLAD_BWD_WAVES ? VLAD_BWD_WAVES / K : 1;
    for (int idx = wave; idx < K * TS; idx += VLAD_BWD_WAVES) {
        const int k = idx / TS, t_first = idx - k * TS;
        float dot = 0.f;
        for (int j = lane; j < HO; j += 64) dot = __fmaf_rn(yb[(int64_t)k * HO + j], dyb[(int64_t)k * HO + j], dot);
        dot = wave_sum(dot);                                // U_k . dU_k (the two sqrt(K) cancel)
        const float rk = r[(int64_t)b * K + k];
        const bool live = rk < VLAD_RMAX;                   // |V_k|^2 was above the epsilon: the projection applies
        float dv[NJ], ck[NJ];
#pragma unroll
        for (int i = 0; i < NJ; ++i) {
            const int j = lane + 64 * i;
            dv[i] = ck[i] = 0.f;
            if (j < HO) {
                const float du = dyb[(int64_t)k * HO + j] * isk, u = yb[(int64_t)k * HO + j] * sk;
                dv[i] = live ? rk * (du - u * dot) : rk * du;
                ck[i] = c[(int64_t)k * HO + j];
                if (t_first == 0) dvb[(int64_t)k * HO + j] = dv[i];
            }
        }
        for (int t = t_first; t < L; t += TS) {
            float p = 0.f;
#pragma unroll
            for (int i = 0; i < NJ; ++i) {
                const int j = lane + 64 * i;
                if (j < HO) p = __fmaf_rn(dv[i], hb[(int64_t)t * HO + j] - ck[i], p);
            }
            p = wave_sum(p);
            if (lane == 0) dsb[(int64_t)t * K + k] = p;
        }
    }
    __syncthreads();                                        // da (in ds) and dV (in dcp) are read back below
    if (tid < K) {                                          // m_k, t ascending
        float m = 0.f;
        for (int t = 0; t < L; ++t) m += ab[(int64_t)t * K + tid];
        ms[tid] = m;
    }
    // the softmax's backward: one wave per row, a lane per cluster
    for (int t = wave; t < T; t += VLAD_BWD_WAVES) {
        float g = 0.f;
        if (t < L) {
            const float w = lane < K ? ab[(int64_t)t * K + lane] : 0.f;
            const float da = lane < K ? dsb[(int64_t)t * K + lane] : 0.f;
            g = w * (da - wave_sum(w * da));
        }
        if (lane < K) dsb[(int64_t)t * K + lane] = g;
    }
    // dh_t = sum_k a_tk dV_k: a thread per column, VLAD_SLAB steps in registers, k ascending; the groups of 256 threads take
    // consecutive step slabs
    float* dhb = dh + (int64_t)b * T * HO;
    const int grp = tid / VLAD_THREADS, ct = tid - grp * VLAD_THREADS;
    for (int r0 = 0; r0 < T; r0 += VLAD_BWD_GROUPS * VLAD_SLAB) {
        const int t0 = r0 + grp * VLAD_SLAB;
        if (r0 >= L) {                                      // (uniform) a round of dead slabs: zeros
            for (int tt = 0; tt < VLAD_SLAB && t0 + tt < T; ++tt)
                for (int col = ct; col < HO; col += VLAD_THREADS) dhb[(int64_t)(t0 + tt) * HO + col] = 0.f;
            continue;
        }
        __syncthreads();                                    // the round before this one has been read
        for (int i = ct; i < K * VLAD_SLAB; i += VLAD_THREADS) {
            const int k = i / VLAD_SLAB, tt = i - k * VLAD_SLAB;
            as[grp][i] = t0 + tt < L ? ab[(int64_t)(t0 + tt) * K + k] : 0.f;
        }
        __syncthreads();
        if (t0 >= T) continue;                              // (no barrier below in this round)
        for (int col = ct; col < HO; col += VLAD_THREADS) {
            float acc[VLAD_SLAB];
#pragma unroll
            for (int tt = 0; tt < VLAD_SLAB; ++tt) acc[tt] = 0.f;
#pragma unroll 4
            for (int k = 0; k < K; ++k) {
                const float v = dvb[(int64_t)k * HO + col];
#pragma unroll
                for (int tt = 0; tt < VLAD_SLAB; ++tt) acc[tt] = __fmaf_rn(as[grp][k * VLAD_SLAB + tt], v, acc[tt]);
            }
#pragma unroll
            for (int tt = 0; tt < VLAD_SLAB; ++tt)
                if (t0 + tt < T) dhb[(int64_t)(t0 + tt) * HO + col] = t0 + tt < L ? acc[tt] : 0.f;
        }
    }
    __syncthreads();                                        // every read of dV is done (and ms is written): dcp = -m_k dV_k in place
    for (int idx = tid; idx < K * HO; idx += VLAD_BWD_THREADS) dvb[idx] *= -ms[idx / HO];
}

static int vlad_check(const char* who, int batch, int T, int HO, int K) {
    VL_CHECK(batch > 0, "%s: batch %d must be positive", who, batch);
    VL_CHECK(K >= 2 && K <= VLAD_MAX_K, "%s: K %d is outside 2..%d (one wave does a row's softmax, a lane per cluster)", who, K,
             VLAD_MAX_K);
    VL_CHECK(HO >= 1 && HO <= VLAD_MAX_HO, "%s: HO %d is outside 1..%d", who, HO, VLAD_MAX_HO);
    VL_CHECK(K * HO <= VLAD_MAX_KHO, "%s: K * HO = %d exceeds %d", who, K * HO, VLAD_MAX_KHO);
    VL_CHECK(T >= 1 && T <= VLAD_MAX_T, "%s: T %d is outside 1..%d (a slab of a clip's assignments lives in LDS)", who, T, VLAD_MAX_T);
    return 0;
}

extern "C" int vl_netvlad_fwd(const float* s, const float* c, const float* h, const int32_t* seq_len, float* a, float* r, float* y,
                              int batch, int T, int HO, int K, vl_stream_t stream) {
    VL_CHECK(s && c && h && a && r && y, "vl_netvlad_fwd: null pointer");
    if (vlad_check("vl_netvlad_fwd", batch, T, HO, K)) return 1;
    hipLaunchKernelGGL(netvlad_fwd_kernel, dim3(batch), dim3(VLAD_THREADS), 0, (hipStream_t)stream, s, c, h, seq_len, a, r, y, T, HO, K);
    VL_LAUNCH_CHECK();
    return 0;
}

extern "C" int vl_netvlad_bwd(const float* dy, const float* h, const float* a, const float* r, const float* y, const float* c,
                              const int32_t* seq_len, float* ds, float* dh, float* dcp, int batch, int T, int HO, int K,
                              vl_stream_t stream) {
    VL_CHECK(dy && h && a && r && y && c && ds && dh && dcp, "vl_netvlad_bwd: null pointer");
    if (vlad_check("vl_netvlad_bwd", batch, T, HO, K)) return 1;
    hipLaunchKernelGGL(netvlad_bwd_kernel, dim3(batch), dim3(VLAD_BWD_THREADS), 0, (hipStream_t)stream, dy, h, a, r, y, c, seq_len, ds, dh,
                       dcp, T, HO, K);
    VL_LAUNCH_CHECK();
    return 0;
}
