// Shared helpers for libvltf_hip.so (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stddef.h>

#include "../../include/vltf.h"

// ---- error convention: int return + thread-local message (include/vltf.h) ----------------------
void vl_set_error(const char* fmt, ...);

#define VL_CHECK(cond, ...)                \
    do {                                   \
        if (!(cond)) {                     \
            vl_set_error(__VA_ARGS__);     \
            return 1;                      \
        }                                  \
    } while (0)

#define VL_HIP(expr)                                                                             \
    do {                                                                                         \
        hipError_t e_ = (expr);                                                                  \
        if (e_ != hipSuccess) {                                                                  \
            vl_set_error("%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, __LINE__); \
            return 2;                                                                            \
        }                                                                                        \
    } while (0)

#define VL_LAUNCH_CHECK() VL_HIP(hipGetLastError())

// ---- experiment / A-B switches -----------------------------------------------------------------
// Every such switch is an environment variable read through this helper into a `static const` (once per process).  The product build
// answers "unset" without looking at the environment; `VL_EXPERIMENTS=1 bash build.sh` builds libvltf_hip_exp.so with them compiled in
// (tools/: VLTF_HIP_LIB=.../libvltf_hip_exp.so).  Nothing in tests/, bench.py or the package depends on one.
#include <stdlib.h>
static inline const char* vl_exp_env(const char* name) {
#ifdef VL_EXPERIMENTS
    return getenv(name);
#else
    (void)name;
    return nullptr;
#endif
}

// ---- division by a runtime constant: q = (mulhi(n, m) + n) >> s, valid for n < 2^31 -------------
struct FastDiv {
    uint32_t d, m, s;
};

static inline FastDiv make_fastdiv(uint32_t d) {
    FastDiv f;
    f.d = d;
    uint32_t s = 0;
    while ((1ull << s) < d) ++s;
    f.s = s;
    f.m = (uint32_t)(((1ull << 32) * ((1ull << s) - d)) / d + 1);
    return f;
}

__device__ __forceinline__ uint32_t fd_div(uint32_t n, const FastDiv& f) { return (__umulhi(n, f.m) + n) >> f.s; }

static inline int ceil_div(int64_t a, int64_t b) { return (int)((a + b - 1) / b); }

// compute units of the current device (256 on MI355X), cached per translation unit: launch plans that size a grid to "one round of
// workgroups" take it from here, not from a literal
static inline int vl_device_cus() {
    static int cus = 0;
    if (!cus) {
        int dev = 0;
        hipDeviceProp_t prop;
        cus = (hipGetDevice(&dev) == hipSuccess && hipGetDeviceProperties(&prop, dev) == hipSuccess && prop.multiProcessorCount > 0)
                  ? prop.multiProcessorCount : 256;
    }
    return cus;
}

// one 64-lane wavefront reductions (gfx950: wave = 64)
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
    return v;
}

// ---- CutMix box (vl_cutmix_pairs in pointwise.hip, vl_cutmix_pairs_s2d in conv_c8.hip) ---------------------------------
// {t0, t1, y0, y1, x0, x1}, half-open.  A launch takes it by value (a checked host box) or reads six device words when it runs.
struct vl_cut_box {
    int v[6];
};

// The box a kernel works on: every bound clamped to its axis [0, n], so that no content of the device words reaches an address;
// false when an axis is then empty (reversed ranges included).  Wave-uniform: the words are the same for every thread.
__device__ __forceinline__ bool cut_box_get(const vl_cut_box& arg, const int32_t* __restrict__ dev, int fpc, int H, int W, int (&b)[6]) {
    const int lim[3] = {fpc, H, W};
#pragma unroll
    for (int i = 0; i < 6; ++i) {
        const int v = dev ? dev[i] : arg.v[i];
        b[i] = v < 0 ? 0 : (v > lim[i >> 1] ? lim[i >> 1] : v);
    }
    return b[0] < b[1] && b[2] < b[3] && b[4] < b[5];
}

// host side of both launches: six host ints inside [0, fpc] x [0, H] x [0, W], no reversed range
static inline int cut_box_host_check(const int32_t* box, int fpc, int H, int W, const char* who, vl_cut_box* out) {
    const int lim[3] = {fpc, H, W};
    static const char* const axis[3] = {"t", "y", "x"};
    for (int a = 0; a < 3; ++a) {
        const int lo = box[2 * a], hi = box[2 * a + 1];
        VL_CHECK(lo >= 0 && hi <= lim[a], "%s: the box's %s range [%d, %d) leaves [0, %d]", who, axis[a], lo, hi, lim[a]);
        VL_CHECK(lo <= hi, "%s: the box's %s range [%d, %d) is reversed", who, axis[a], lo, hi);
        out->v[2 * a] = lo;
        out->v[2 * a + 1] = hi;
    }
    return 0;
}

// ---- counter-based draws (dropout in pointwise.hip, random erasing below) -----------------------------------------------------------
__device__ __forceinline__ uint64_t splitmix64(uint64_t z) {
    z += 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

// ---- dropout of the self-attention model (vl_mhsa_drop_*, vl_add_layer_norm_drop_fwd, vl_branch_drop_grad; vltf.h) -----
// The generator of vl_fc_dropout_fwd under a stream constant of its own: SA_DROP_STREAM + salt is above 2^45 for every 32-bit salt, so
// no stream here is one of 0xFC00 + salt, and vl_dropout_fwd uses the bare seed.  What a launch draws with: the seed (st NULL) or the
// step state it is formed from when the kernel runs, and the index in the whole batch of the launch's first clip.
#define SA_DROP_STREAM 0x5AD000000000ull
struct SaDraw {
    uint64_t seed;
    const vl_step_state* st;
    int64_t clip0;
};
__device__ __forceinline__ uint64_t sa_drop_stream(const SaDraw& dw, uint32_t salt) {
    const uint64_t seed = dw.st ? (((uint64_t)dw.st->step << 20) ^ 0x5DEECE66Dull) : dw.seed;
    return seed ^ splitmix64(SA_DROP_STREAM + (uint64_t)salt);
}
__device__ __forceinline__ bool sa_drop_kept(uint64_t s, uint64_t e, float keep) {
    const uint64_t h = splitmix64(s ^ splitmix64(e));
    return (float)(h >> 40) * (1.0f / 16777216.0f) < keep;
}
// the factor of a branch element: fe = kept_e ? 1 / keep : 0, fp = path_kept ? 1 / keep_path : 0, f = fe * fp; a keep of 1 draws nothing
// and gives exactly 1.  se / sp: the element and path streams; e: the element's counter, pe: the path counter 2 * clip + branch.
__device__ __forceinline__ float sa_path_factor(uint64_t sp, uint64_t pe, float keep_path) {
    return keep_path < 1.f ? (sa_drop_kept(sp, pe, keep_path) ? __fdiv_rn(1.0f, keep_path) : 0.f) : 1.f;
}
__device__ __forceinline__ float sa_branch_factor(uint64_t se, uint64_t e, float keep, float inv_keep, float fp) {
#pragma clang fp contract(off)
    const float fe = keep < 1.f ? (sa_drop_kept(se, e, keep) ? inv_keep : 0.f) : 1.f;
    return fe * fp;
}
// s = fadd(x, fmul(r, f)), never an fma
__device__ __forceinline__ float sa_branch_add(float x, float r, float f) {
#pragma clang fp contract(off)
    const float rf = r * f;
    return x + rf;
}
static inline bool sa_keep_ok(float keep) { return keep > 0.f && keep <= 1.f; }      // (false for NaN)

// ---- random erasing (vl_erase_boxes in pointwise.hip, vl_erase_boxes_s2d in conv_c8.hip) -------------------------------
// A clip's row of the device table: {t0, t1, y0, y1, x0, x1, key_lo, key_hi}.  The box is clamped as a CutMix box is (cut_box_get), so
// no content of the words reaches an address; false when an axis is then empty.  Wave-uniform.
#define ERASE_ROW_WORDS 8
#define ERASE_CLIP_ELEMENT (1ull << 40)          // mode 1: the element of channel c is 2^40 + c, above every pixel index of mode 2
__device__ __forceinline__ bool erase_row_get(const int32_t* __restrict__ row, int fpc, int H, int W, int (&b)[6], uint64_t& key) {
    const vl_cut_box none = {{0, 0, 0, 0, 0, 0}};
    key = ((uint64_t)(uint32_t)row[7] << 32) | (uint64_t)(uint32_t)row[6];
    return cut_box_get(none, row, fpc, H, W, b);
}

// host side of both launches: neither NaN nor an infinity (v - v is 0 for every finite v and NaN otherwise)
static inline bool erase_scale_ok(float v) { return v - v == 0.f; }

// noise(key, e): the four 16-bit fields of one hash summed (an Irwin-Hall sum: mean 131070, standard deviation 37837.227...), centred
// as an integer, then ONE fp32 multiply -- a host restatement in integers and one fp32 product gives the same bits.
__device__ __forceinline__ float erase_noise(uint64_t key, uint64_t e, float scale) {
    const uint64_t h = splitmix64(key ^ splitmix64(e));
    const int s = (int)(h & 0xffffu) + (int)((h >> 16) & 0xffffu) + (int)((h >> 32) & 0xffffu) + (int)(h >> 48);
    return (float)(s - 131070) * scale;
}

// ---- random resized crop (vl_input_prep_u8_box in pointwise.hip, vl_input_prep_u8_box_s2d in conv_c8.hip) --------------
// A frame's box {y0, x0, bh, bw} as a kernel uses it: sizes clamped into [1, raw] first, then the corner into [0, raw - size], so
// that no content of the device words reaches an address outside the frame.
struct BoxRect {
    int y0, x0, bh, bw;
};
__device__ __forceinline__ BoxRect box_get(const int32_t* __restrict__ box, int img, int rh, int rw) {
    const int32_t* b = box + 4 * (int64_t)img;
    BoxRect r;
    r.bh = min(max(b[2], 1), rh);
    r.bw = min(max(b[3], 1), rw);
    r.y0 = min(max(b[0], 0), rh - r.bh);
    r.x0 = min(max(b[1], 0), rw - r.bw);
    return r;
}

// One axis of the bilinear rule (half-pixel centres, clamped to the box's edge): output index o of `out` over a box side of b pixels.
// num = max((2 o + 1) b - out, 0) is 2 out times the source coordinate; taps i0 <= i1 and the weight of i1, all from integers.
// Where both taps are the same pixel (a clamped edge) the weight is immaterial and taken as 0: the sample is then that pixel exactly.
struct BoxTap {
    int i0, i1;
    float f;
};
__device__ __forceinline__ BoxTap box_tap(int o, int b, int out, const FastDiv& d2out) {
    const uint32_t num = (uint32_t)max((2 * o + 1) * b - out, 0);
    const uint32_t q = fd_div(num, d2out), r = num - q * (2u * (uint32_t)out);
    BoxTap t;
    t.i0 = min((int)q, b - 1);
    t.i1 = min((int)q + 1, b - 1);
    t.f = t.i0 == t.i1 ? 0.f : __fdiv_rn((float)r, (float)(2 * out));
    return t;
}

// lerp(a, b, f) = a (1 - f) + b f in this one order of roundings, for both kernels
__device__ __forceinline__ float box_lerp(float a, float b, float f) { return __fmaf_rn(b, f, __fmul_rn(a, __fsub_rn(1.f, f))); }

// The sample: r0 / r1 point at the channel's byte of column 0 of the two tap rows, o0 / o1 are the byte offsets of the two tap
// columns.  Horizontal lerps first, then the vertical one, then the mean.
__device__ __forceinline__ float box_sample(const uint8_t* __restrict__ r0, const uint8_t* __restrict__ r1, int o0, int o1, float fx,
                                            float fy, float mean) {
    const float top = box_lerp((float)r0[o0], (float)r0[o1], fx);
    const float bot = box_lerp((float)r1[o0], (float)r1[o1], fx);
    return __fsub_rn(box_lerp(top, bot, fy), mean);
}

// ---- LSTM recurrence: per-clip form (pointwise.hip), the fallback / A-B reference of the cluster form (lstm_cluster.hip) ------
int vl_lstm_perclip_fwd(const float* gx, const float* kh, const float* h0, const float* c0, float* act, float* cseq, float* hseq,
                        float* hprev, int batch, int T, int H, float forget_bias, const int32_t* seq_len, hipStream_t stream);
int vl_lstm_perclip_bwd(const float* dout, const float* kh_t, const float* act, const float* cseq, const float* c0, float* dz,
                        float* dh0, float* dc0, int batch, int T, int H, const int32_t* seq_len, hipStream_t stream);
