// HBM-bound kernels of the LRCN path: input prep, LRN, max-pool, bias/column sums, LSTM gate
// pointwise, temporal fusion, dropout, softmax cross-entropy, global-norm + SGD/Adam.
// All activations NCHW fp32; lanes always walk the contiguous (w / hw / column) dimension.
#include <stdlib.h>

#include <stdio.h>
#include <stdlib.h>

#include "common.h"

// A/B switches for measurements, read once: VL_POOL_LRN_CHUNKED=1 runs the fused pool+LRN backward on the older chunked
// kernel, VL_POOL_LRN_CHK16=1 forces the 16-channel chunk of the channel-stream kernel.
static const bool kPoolLrnChunked = vl_exp_env("VL_POOL_LRN_CHUNKED") != nullptr;
static const bool kPoolLrnChk16 = vl_exp_env("VL_POOL_LRN_CHK16") != nullptr;
static const bool kMaxpoolGeneric = vl_exp_env("VL_MAXPOOL_GENERIC") != nullptr;   // A/B: pool5 backward, element-per-thread kernel

static inline int grid_for(int64_t work, int threads, int cap) {
    int64_t b = (work + threads - 1) / threads;
    if (b > cap) b = cap;
    if (b < 1) b = 1;
    return (int)b;
}

// ---- input prep (dataset_.py:481-501) ---------------------------------------------------------
// Threads walk the DESTINATION plane by plane: thread -> (phase plane ph, row y, column q of the plane), an image per blockIdx.y.  The
// interior rows of a (channel, phase) plane are one contiguous run when every column of a row is written -- the halo / padding columns
// too, as the 0.0 they hold by contract -- so a wave's stores are whole 256-byte runs in each of the three channel planes.  (Round 1 -
// 3: (row, phase, column) order with the halo columns skipped: 236-byte row pieces, every piece's end sectors written partially, and
// three 64-bit divisions per element; 0.25 ms per 1024 frames = 3.1 TB/s.)  The source bytes of a wave are `phase` pixels apart (12 B
// at phase 4), all within a few cache lines.
__global__ __launch_bounds__(256) void input_prep_u8_kernel(const uint8_t* __restrict__ src, float* __restrict__ dst, int rh, int rw, int oh,
                                                            int ow, const int32_t* __restrict__ cy, const int32_t* __restrict__ cx,
                                                            const uint8_t* __restrict__ mir, const float* __restrict__ mean, int halo, int phase,
                                                            int wp, FastDiv d_plane, FastDiv d_wp) {
    // phase > 1: column-phase-split destination [c][phase][oh + 2 halo][wp = ceil((ow + 2 halo) / phase)] (vl_conv_set_x_phase_split)
    const int img = blockIdx.y;
    const uint32_t plane_in = (uint32_t)oh * wp, per_img = plane_in * phase;      // interior rows of one plane; of all phase planes
    const int64_t pp = (int64_t)(oh + 2 * halo) * wp;
    const float m0 = mean ? mean[0] : 0.f, m1 = mean ? mean[1] : 0.f, m2 = mean ? mean[2] : 0.f;
    const int oy = cy ? cy[img] : 0, ox = cx ? cx[img] : 0;
    const bool flip = mir && mir[img];
    const uint8_t* simg = src + (int64_t)img * rh * rw * 3;
    float* dimg = dst + (int64_t)img * 3 * phase * pp + (int64_t)halo * wp;
    for (uint32_t e = blockIdx.x * 256u + threadIdx.x; e < per_img; e += gridDim.x * 256u) {
        const uint32_t ph = fd_div(e, d_plane), r = e - ph * plane_in;
        const uint32_t y = fd_div(r, d_wp), q = r - y * wp;
        const int x = (int)(q * phase + ph) - halo;                   // physical column q * phase + ph of the haloed row
        float v0 = 0.f, v1 = 0.f, v2 = 0.f;                           // halo / padding columns: the zeros they hold
        if (x >= 0 && x < ow) {
            const uint8_t* sp = simg + ((int64_t)(y + oy) * rw + (flip ? ow - 1 - x : x) + ox) * 3;
            v0 = (float)sp[0] - m0;
            v1 = (float)sp[1] - m1;
            v2 = (float)sp[2] - m2;
        }
        float* d = dimg + (int64_t)ph * pp + r;                        // r = y * wp + q: the plane's interior rows are contiguous
        d[0] = v0;
        d[(int64_t)phase * pp] = v1;
        d[2 * (int64_t)phase * pp] = v2;
    }
}

extern "C" int vl_input_prep_u8(const uint8_t* src, float* dst, int n, int raw_h, int raw_w, int out_h, int out_w,
                                const int32_t* crop_y, const int32_t* crop_x, const uint8_t* mirror, const float* mean_bgr,
                                int dst_halo, int dst_phase, vl_stream_t stream) {
    VL_CHECK(src && dst && dst_halo >= 0 && dst_phase >= 1, "vl_input_prep_u8: bad argument");
    VL_CHECK(n > 0 && out_h > 0 && out_w > 0 && out_h <= raw_h && out_w <= raw_w, "vl_input_prep_u8: bad shape");
    VL_CHECK(n <= 65535, "vl_input_prep_u8: batch %d exceeds the grid limit", n);
    const int wp = (out_w + 2 * dst_halo + dst_phase - 1) / dst_phase;
    const int64_t per_img = (int64_t)out_h * dst_phase * wp;
    VL_CHECK(per_img < (1ll << 31), "vl_input_prep_u8: image too large");
    int bx = (int)((per_img + 1023) / 1024);                          // ~4 elements per thread
    if ((int64_t)bx * n < 8ll * vl_device_cus()) bx = (int)((per_img + 255) / 256);   // few frames: one element per thread
    hipLaunchKernelGGL(input_prep_u8_kernel, dim3(bx, n), dim3(256), 0, (hipStream_t)stream, src, dst, raw_h, raw_w, out_h, out_w,
                       crop_y, crop_x, mirror, mean_bgr, dst_halo, dst_phase, wp, make_fastdiv((uint32_t)out_h * wp), make_fastdiv((uint32_t)wp));
    VL_LAUNCH_CHECK();
    return 0;
}

// ---- input prep with a box per frame: random resized crop ------------------------------------------------------------
// input_prep_u8_kernel's destination walk (thread -> (phase plane, row, plane column), whole store runs, an image per blockIdx.y); the
// source is the frame's own box {y0, x0, bh, bw}, resampled bilinearly to oh x ow by the rule of common.h (box_tap / box_sample): four
// byte taps per channel where the crop reads one.  The taps' quotients are FastDiv by the launch-uniform 2 oh and 2 ow; the box is
// clamped into the frame before any address is formed (box_get).
__global__ __launch_bounds__(256) void input_prep_u8_box_kernel(const uint8_t* __restrict__ src, float* __restrict__ dst, int rh, int rw,
                                                                int oh, int ow, const int32_t* __restrict__ box,
                                                                const uint8_t* __restrict__ mir, const float* __restrict__ mean, int halo,
                                                                int phase, int wp, FastDiv d_plane, FastDiv d_wp, FastDiv d_2oh,
                                                                FastDiv d_2ow) {
    const int img = blockIdx.y;
    const uint32_t plane_in = (uint32_t)oh * wp, per_img = plane_in * phase;
    const int64_t pp = (int64_t)(oh + 2 * halo) * wp;
    const float m0 = mean ? mean[0] : 0.f, m1 = mean ? mean[1] : 0.f, m2 = mean ? mean[2] : 0.f;
    const BoxRect b = box_get(box, img, rh, rw);
    const bool flip = mir && mir[img];
    const int pitch = rw * 3;
    const uint8_t* sbox = src + (int64_t)img * rh * pitch + (int64_t)b.y0 * pitch + b.x0 * 3;       // the box's first pixel
    float* dimg = dst + (int64_t)img * 3 * phase * pp + (int64_t)halo * wp;
    for (uint32_t e = blockIdx.x * 256u + threadIdx.x; e < per_img; e += gridDim.x * 256u) {
        const uint32_t ph = fd_div(e, d_plane), r = e - ph * plane_in;
        const uint32_t y = fd_div(r, d_wp), q = r - y * wp;
        const int x = (int)(q * phase + ph) - halo;
        float v0 = 0.f, v1 = 0.f, v2 = 0.f;
        if (x >= 0 && x < ow) {
            const BoxTap ty = box_tap((int)y, b.bh, oh, d_2oh), tx = box_tap(flip ? ow - 1 - x : x, b.bw, ow, d_2ow);
            const uint8_t *r0 = sbox + ty.i0 * pitch, *r1 = sbox + ty.i1 * pitch;
            const int o0 = tx.i0 * 3, o1 = tx.i1 * 3;
            v0 = box_sample(r0, r1, o0, o1, tx.f, ty.f, m0);
            v1 = box_sample(r0 + 1, r1 + 1, o0, o1, tx.f, ty.f, m1);
            v2 = box_sample(r0 + 2, r1 + 2, o0, o1, tx.f, ty.f, m2);
        }
        float* d = dimg + (int64_t)ph * pp + r;
        d[0] = v0;
        d[(int64_t)phase * pp] = v1;
        d[2 * (int64_t)phase * pp] = v2;
    }
}

extern "C" int vl_input_prep_u8_box(const uint8_t* src, float* dst, int n, int raw_h, int raw_w, int out_h, int out_w, const int32_t* box,
                                    const uint8_t* mirror, const float* mean_bgr, int dst_halo, int dst_phase, vl_stream_t stream) {
    VL_CHECK(src && dst && box && dst_halo >= 0 && dst_phase >= 1, "vl_input_prep_u8_box: bad argument");
    VL_CHECK(n > 0 && out_h > 0 && out_w > 0 && raw_h > 0 && raw_w > 0, "vl_input_prep_u8_box: bad shape");
    VL_CHECK(n <= 65535, "vl_input_prep_u8_box: batch %d exceeds the grid limit", n);
    // the taps' numerators (2 o + 1) b and a frame's byte offsets stay inside 31 bits
    VL_CHECK((2ll * out_h + 1) * raw_h < (1ll << 31) && (2ll * out_w + 1) * raw_w < (1ll << 31) && 3ll * raw_h * raw_w < (1ll << 31),
             "vl_input_prep_u8_box: image too large");
    const int wp = (out_w + 2 * dst_halo + dst_phase - 1) / dst_phase;
    const int64_t per_img = (int64_t)out_h * dst_phase * wp;
    VL_CHECK(per_img < (1ll << 31), "vl_input_prep_u8_box: image too large");
    int bx = (int)((per_img + 1023) / 1024);
    if ((int64_t)bx * n < 8ll * vl_device_cus()) bx = (int)((per_img + 255) / 256);
    hipLaunchKernelGGL(input_prep_u8_box_kernel, dim3(bx, n), dim3(256), 0, (hipStream_t)stream, src, dst, raw_h, raw_w, out_h, out_w, box,
                       mirror, mean_bgr, dst_halo, dst_phase, wp, make_fastdiv((uint32_t)out_h * wp), make_fastdiv((uint32_t)wp),
                       make_fastdiv(2u * (uint32_t)out_h), make_fastdiv(2u * (uint32_t)out_w));
    VL_LAUNCH_CHECK();
    return 0;
}

// generic 3-level strided copy: dst[(a*nb + b)*nc + c] = src[a*sa + b*sb + c*sc]
__global__ void permute3_kernel(const float* __restrict__ src, float* __restrict__ dst, int64_t na, int nb, int nc, int64_t sa,
                                int64_t sb, int64_t sc) {
    const int64_t total = na * nb * nc;
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (int64_t)gridDim.x * blockDim.x) {
        const int c = (int)(e % nc);
        const int b = (int)((e / nc) % nb);
        const int64_t a = e / ((int64_t)nc * nb);
        dst[e] = src[a * sa + b * sb + c * sc];
    }
}

__global__ void nhwc_to_nchw_halo_kernel(const float* __restrict__ src, float* __restrict__ dst, int n, int h, int w, int c,
                                         int halo, int phase) {
    const int64_t total = (int64_t)n * c * h * w;
    const int wp = (w + 2 * halo + phase - 1) / phase;
    const int64_t pp = (int64_t)(h + 2 * halo) * wp;
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (int64_t)gridDim.x * blockDim.x) {
        const int x = (int)(e % w);
        const int y = (int)((e / w) % h);
        const int ch = (int)((e / ((int64_t)w * h)) % c);
        const int64_t img = e / ((int64_t)w * h * c);
        const int xc = x + halo;
        dst[((img * c + ch) * phase + xc % phase) * pp + (int64_t)(y + halo) * wp + xc / phase] = src[((img * h + y) * w + x) * c + ch];
    }
}

extern "C" int vl_nhwc_to_nchw(const float* src, float* dst, int n, int h, int w, int c, int dst_halo, int dst_phase,
                               vl_stream_t stream) {
    VL_CHECK(src && dst && n > 0 && h > 0 && w > 0 && c > 0 && dst_halo >= 0 && dst_phase >= 1, "vl_nhwc_to_nchw: bad argument");
    hipLaunchKernelGGL(nhwc_to_nchw_halo_kernel, dim3(grid_for((int64_t)n * h * w * c, 256, 8192)), dim3(256), 0, (hipStream_t)stream,
                       src, dst, n, h, w, c, dst_halo, dst_phase);
    VL_LAUNCH_CHECK();
    return 0;
}

extern "C" int vl_nchw_to_nhwc(const float* src, float* dst, int n, int c, int h, int w, vl_stream_t stream) {
    VL_CHECK(src && dst && n > 0 && h > 0 && w > 0 && c > 0, "vl_nchw_to_nhwc: bad argument");
    const int64_t hw = (int64_t)h * w;
    hipLaunchKernelGGL(permute3_kernel, dim3(grid_for(n * hw * c, 256, 8192)), dim3(256), 0, (hipStream_t)stream, src, dst,
                       (int64_t)n, (int)hw, c, hw * c, (int64_t)1, hw);
    VL_LAUNCH_CHECK();
    return 0;
}

// ---- LRN across channels (alexnet.py:79-89) ---------------------------------------------------
// One thread = one (image, pixel) column x CH consecutive channels; lanes walk pixels, so every
// load is a coalesced row of a channel plane.  The window lives in registers (static unroll).
__device__ __forceinline__ float pow_neg(float v, float beta) {
    // v >= bias > 0.  beta = 0.75 (the only value the reference uses) maps to two 1-ulp ops.
    if (beta == 0.75f) {
        const float r = __builtin_amdgcn_rsqf(v);
        return r * __builtin_amdgcn_sqrtf(r);
    }
    return powf(v, -beta);
}

template <int CH, int R>
__global__ void lrn_fwd_kernel(const float* __restrict__ x, float* __restrict__ y, int n, int C, int HW, float alpha, float beta,
                               float bias) {
    const int64_t pos = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (pos >= (int64_t)n * HW) return;
    const int img = (int)(pos / HW);
    const int p = (int)(pos - (int64_t)img * HW);
    const int c0 = blockIdx.y * CH;
    const float* xp = x + (int64_t)img * C * HW + p;
    float* yp = y + (int64_t)img * C * HW + p;
    float v[CH + 2 * R];
#pragma unroll
    for (int i = 0; i < CH + 2 * R; ++i) {
        const int c = c0 - R + i;
        v[i] = (c >= 0 && c < C) ? xp[(int64_t)c * HW] : 0.f;
    }
#pragma unroll
    for (int i = 0; i < CH; ++i) {
        if (c0 + i < C) {
            float s = 0.f;
#pragma unroll
            for (int d = 0; d <= 2 * R; ++d) s += v[i + d] * v[i + d];
            yp[(int64_t)(c0 + i) * HW] = v[i + R] * pow_neg(bias + alpha * s, beta);
        }
    }
}

template <int CH, int R>
__global__ void lrn_bwd_kernel(const float* __restrict__ x, const float* __restrict__ dy, float* __restrict__ dx, int n, int C,
                               int HW, float alpha, float beta, float bias, int relu_fused, int W, int halo) {
    const int64_t pos = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (pos >= (int64_t)n * HW) return;
    const int img = (int)(pos / HW);
    const int p = (int)(pos - (int64_t)img * HW);
    const int c0 = blockIdx.y * CH;
    const int64_t off = (int64_t)img * C * HW + p;
    const float* xp = x + off;
    const float* gp = dy + off;
    float xv[CH + 4 * R];  // channels c0-2R .. c0+CH+2R-1
#pragma unroll
    for (int i = 0; i < CH + 4 * R; ++i) {
        const int c = c0 - 2 * R + i;
        xv[i] = (c >= 0 && c < C) ? xp[(int64_t)c * HW] : 0.f;
    }
    // dx may carry a halo: plane pitch (H + 2 halo)(W + 2 halo), interior origin at (halo, halo)
    const int py = p / W, px = p - py * W;
    const int wp = W + 2 * halo;
    const int64_t dpp = (int64_t)(HW / W + 2 * halo) * wp;
    float* dxp = dx + (int64_t)img * C * dpp + (int64_t)(py + halo) * wp + px + halo;
    float t[CH + 2 * R];  // dy_c * x_c * s_c^(-beta-1) for c0-R .. c0+CH+R-1
    float u[CH];          // s_c^-beta for the owned channels
#pragma unroll
    for (int i = 0; i < CH + 2 * R; ++i) {
        const int c = c0 - R + i;
        float s = 0.f;
#pragma unroll
        for (int d = 0; d <= 2 * R; ++d) s += xv[i + d] * xv[i + d];
        const float sc = bias + alpha * s;
        const float pw = pow_neg(sc, beta);
        const float g = (c >= 0 && c < C) ? gp[(int64_t)c * HW] : 0.f;
        t[i] = g * xv[i + R] * pw * __builtin_amdgcn_rcpf(sc);
        if (i >= R && i < CH + R) u[i - R] = g * pw;
    }
#pragma unroll
    for (int i = 0; i < CH; ++i) {
        if (c0 + i < C) {
            float a = 0.f;
#pragma unroll
            for (int d = 0; d <= 2 * R; ++d) a += t[i + d];
            const float xc = xv[i + 2 * R];
            float r = u[i] - 2.f * alpha * beta * xc * a;
            if (relu_fused) r = xc > 0.f ? r : 0.f;
            dxp[(int64_t)(c0 + i) * dpp] = r;
        }
    }
}

// Fused max-pool(3x3/2 VALID) backward + LRN backward (+ReluGrad): the gradient wrt the LRN output is
// never materialised.  One thread = one (image, pixel) column x CH channels.  The <= 4 pooling windows
// that contain the pixel are the same for every channel, so they are decoded once; per channel the
// routed gradient is a <= 4-term gather from the (tiny, cache resident) pooled gradient + arg-max maps.
// One workgroup = (image, CH-channel chunk, band of 2*PR input rows).  The pooled gradient and the arg-max
// bytes that band can touch ((PR+1) pooled rows x CH+2R channels: ~20 KB) are staged in LDS with coalesced
// loads; every per-pixel gather then hits LDS, never the texture path (a per-pixel global gather version
// was TA-bound at 3.5-6 ms for lrn1).
template <int CH, int R, int NPIX>
__global__ __launch_bounds__(256) void pool_lrn_bwd_kernel(const float* __restrict__ x, const float* __restrict__ dp,
                                                           const uint8_t* __restrict__ arg, float* __restrict__ dx, int C, int H,
                                                           int W, int OH, int OW, int64_t ps_n, int ps_c, int ps_h, float alpha,
                                                           float beta, float bias, int relu_fused, int halo) {
    constexpr int NC = CH + 2 * R;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int HW = H * W;
    const int img = blockIdx.z, c0 = blockIdx.y * CH;
    const int p0 = blockIdx.x * NPIX;                                 // band = NPIX consecutive pixels of the plane
    const int npix = min(NPIX, HW - p0);
    const int r0 = p0 / W, r1 = (p0 + npix - 1) / W;                  // input rows the band touches
    const int oh0 = (r0 >> 1) - 1;                                    // first pooled row that can reach the band
    const int prow = (r1 >> 1) - oh0 + 1;                             // pooled rows staged
    const int rowlen = prow * OW;
    float* sdp = reinterpret_cast<float*>(smem);                      // [NC][prow][OW]
    uint8_t* sarg = smem + (size_t)NC * rowlen * sizeof(float);       // [NC][prow][OW]
    const float* dpp = dp + (int64_t)img * ps_n;
    const uint8_t* ap = arg + (int64_t)img * ps_n;
    for (int e = threadIdx.x; e < NC * rowlen; e += 256) {
        const int ci = e / rowlen, rem = e - ci * rowlen;
        const int rr = rem / OW, ow = rem - rr * OW;
        const int c = c0 - R + ci, oh = oh0 + rr;
        const bool ok = c >= 0 && c < C && oh >= 0 && oh < OH;
        const int o = ok ? c * ps_c + oh * ps_h + ow : 0;
        sdp[e] = ok ? dpp[o] : 0.f;
        sarg[e] = ok ? ap[o] : (uint8_t)255;                           // 255 never equals a window-local index
    }
    __syncthreads();
    const float* xim = x + (int64_t)img * C * HW;
    const int wp = W + 2 * halo;
    const int64_t dplane = (int64_t)(H + 2 * halo) * wp;
    float* dxim = dx + (int64_t)img * C * dplane;
    for (int pix = threadIdx.x; pix < npix; pix += 256) {
        const int py = (p0 + pix) / W, px = (p0 + pix) - py * W;
        // the <= 4 windows (k = 3, s = 2) containing (py, px), as LDS offsets within a channel slab
        int woff[4], wloc[4];
#pragma unroll
        for (int a = 0; a < 2; ++a) {
            const int oh = (py >> 1) - a, lr = (py & 1) + 2 * a;
            const bool rok = oh >= 0 && oh < OH && lr <= 2;
#pragma unroll
            for (int b = 0; b < 2; ++b) {
                const int ow = (px >> 1) - b, lc = (px & 1) + 2 * b;
                const bool ok = rok && ow >= 0 && ow < OW && lc <= 2;
                woff[a * 2 + b] = ok ? (oh - oh0) * OW + ow : 0;
                wloc[a * 2 + b] = ok ? lr * 3 + lc : 254;              // 254: matches neither a real index nor the 255 filler
            }
        }
        const float* xp = xim + (int64_t)py * W + px;
        float xv[CH + 4 * R];
#pragma unroll
        for (int i = 0; i < CH + 4 * R; ++i) {
            const int c = c0 - 2 * R + i;
            xv[i] = (c >= 0 && c < C) ? xp[(int64_t)c * HW] : 0.f;
        }
        float t[NC], u[CH];
#pragma unroll
        for (int i = 0; i < NC; ++i) {
            float g = 0.f;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int o = i * rowlen + woff[q];
                g += ((int)sarg[o] == wloc[q]) ? sdp[o] : 0.f;
            }
            float s = 0.f;
#pragma unroll
            for (int d = 0; d <= 2 * R; ++d) s += xv[i + d] * xv[i + d];
            const float sc = bias + alpha * s;
            const float pw = pow_neg(sc, beta);
            t[i] = g * xv[i + R] * pw * __builtin_amdgcn_rcpf(sc);
            if (i >= R && i < CH + R) u[i - R] = g * pw;
        }
        float* dxp = dxim + (int64_t)(py + halo) * wp + px + halo;
#pragma unroll
        for (int i = 0; i < CH; ++i) {
            if (c0 + i < C) {
                float a = 0.f;
#pragma unroll
                for (int d = 0; d <= 2 * R; ++d) a += t[i + d];
                const float xc = xv[i + 2 * R];
                float r = u[i] - 2.f * alpha * beta * xc * a;
                if (relu_fused) r = xc > 0.f ? r : 0.f;
                dxp[(int64_t)(c0 + i) * dplane] = r;
            }
        }
    }
}

// ---- the same fused backward as a CHANNEL STREAM (the form the benchmark layers run) ----------------------------------
// One thread = one pixel of one image; it walks ALL channels in order, carrying the LRN windows (5 inputs, 5 t-terms,
// 3 u-terms) in registers, so no channel is re-read or re-computed at chunk edges (the chunked form above reads 24 and
// evaluates 20 channels per 16 outputs), and the x loads of the next 16 channels are in flight while this 16 are computed:
// 16 KB per workgroup outstanding at all times -- the chunked form alternated load-wait and compute phases and reached
// ~40 % of the HBM rate.  The pooled gradient / arg-max of each 16-channel chunk go through LDS (two buffers, one barrier
// per chunk) as 8-byte {dp, arg} entries; the <= 4 pooling windows of a pixel are two adjacent entries in each of two
// pooled rows, i.e. two addresses + an immediate.  x loads / dx stores are buffer accesses with a per-thread constant
// pixel offset and a scalar channel offset: pixels past the plane fail the range check (loads 0, stores dropped).
// Channel cc enters the x window at iteration cc; t[cc-2] is then computable, and the output of channel cc-4.
// (band, image) of a workgroup in XCD-aware order (round 4).  Workgroup ids are dealt round-robin over the 8 XCDs, each with its own L2;
// with the natural order (band fastest) the bands of one image -- which share input rows / pooled rows at their seams, and for the
// backward kernel re-read each pooled row 2.25 times between them -- land on 8 different L2s and every re-read is an HBM fetch
// (measured: 1.44 x the algorithmic bytes fetched, tools/pw_pmc_probe.sh).  Here eight consecutive images take the 8 XCDs and an
// image's bands follow each other on ITS XCD, eight ids apart, i.e. dispatched together.  Grid = (bands, images rounded up to 8, z);
// false = padding.  Placement affects speed only.
__device__ __forceinline__ bool xcd_band_image(int nimg, int& band, int& img) {
    const int nb = gridDim.x;
    const int L = blockIdx.y * nb + blockIdx.x;
    const int g = L / (nb * 8), r = L - g * (nb * 8);
    band = r >> 3;
    img = g * 8 + (r & 7);
    return img < nimg;
}

static constexpr uint32_t PW_OOB = 0xF0000000u;   // fails the range check of every resource built below (sizes < 2^31)

__device__ __forceinline__ __amdgpu_buffer_rsrc_t pw_rsrc(const void* base, int64_t bytes) {
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(base), 0, (int)(uint32_t)bytes, 0x00020000);
}

// C8: dx is the packed-bf16 "c8" gradient [image][C / 8][H + 2 halo][W + 2 halo][8] (conv_c8.hip) instead of fp32 NCHW.  The chunk is
// then 8 channels starting at a multiple of 8: its outputs are channels c0 - 4 .. c0 + 3, i.e. the upper half of one 16-byte chunk and
// the lower half of the next, each stored as ONE 8-byte word per pixel (4 bf16, rounded to nearest even).
// C8 == 2: x (the LRN input = the conv's ReLU output) is packed too, [image][C / 8][H][W][8] bf16 without a halo: one 16-byte load
// per pixel brings a chunk's 8 channels.
template <int CHK, int NST, bool RELU, int C8 = 0>
__global__ __launch_bounds__(256, (C8 ? 3 : 1)) void pool_lrn_bwd_stream_kernel(const float* __restrict__ x, const float* __restrict__ dp,
                                                                  const uint8_t* __restrict__ arg, float* __restrict__ dx, int C,
                                                                  int H, int W, int OH, int OW, int64_t ps_n, int ps_c, int ps_h,
                                                                  int64_t pooled_bytes_f, float alpha, float bias, int halo, int cper, int nimg) {
    constexpr int BUF = NST * 256 + 16;                               // entries per LDS buffer (+ pad: entries -1 and one-past-the-end are read)
    // blockIdx.z owns the OUTPUT channels [R0, R1) (cper channels; the whole tensor when the grid is flat).  Its walk starts LEAD
    // channels earlier with empty windows: what it computes for channels below R0 there is wrong and dropped, and by channel R0 the x
    // window (4 back), the t window (2 more) are complete -- 4 (8: whole packed chunks) extra iterations per range buy workgroups
    // for launches whose (band, image) grid fills the chip 1.5 times (27 x 27 x 256 at 1024 frames) or not at all (128 frames).
    constexpr int LEAD = C8 ? 8 : 4;
    const int R0 = blockIdx.z * cper, R1 = min(C, R0 + cper);
    const int cs = max(R0 - LEAD, 0);                                 // never below channel 0: windows that start there ARE empty
    __shared__ __attribute__((aligned(16))) uint2 stage[2 * BUF];
    const int HW = H * W;
    int band, img;
    if (!xcd_band_image(nimg, band, img)) return;
    // fp32 output in a halo layout: the lanes enumerate WHOLE rows of that layout, halo columns included -- those lanes load nothing
    // (their x and routed gradient are 0, so the value they compute IS the 0.0 a halo holds) and a wave's stores are runs of full
    // sectors instead of 112-byte pieces at a 128-byte pitch (round 4: lrn_pool_fwd's lesson, profiles/r04_lrn_pool_fwd_experiments.txt)
    const int Wq = C8 == 0 ? W + 2 * halo : W, HWq = H * Wq;
    const int p0 = band * 256, p = p0 + threadIdx.x;
    const bool inplane = p < HWq;
    const int pc = inplane ? p : HWq - 1;
    const int py = pc / Wq, pxq = pc - py * Wq, pxr = pxq - (Wq - W) / 2;
    const bool valid = inplane && pxr >= 0 && pxr < W;
    const int px = min(max(pxr, 0), W - 1);
    const int r0 = p0 / Wq, r1 = min(p0 + 255, HWq - 1) / Wq;         // input rows of the band
    const int oh0 = (r0 >> 1) - 1;                                    // first pooled row that can reach the band
    const int prow = (r1 >> 1) - oh0 + 1;
    const int rowlen = prow * OW;

    // ---- per-thread constants of the staging pass: entry e = tid + 256 j  <->  (slab ci, pooled row, pooled column),
    // packed as ci << 24 | (row * pitch + column); -1 = nothing to fetch
    int st[NST];
#pragma unroll
    for (int j = 0; j < NST; ++j) {
        const int e = threadIdx.x + 256 * j;
        const int ci = e / rowlen, rem = e - ci * rowlen;
        const int rr = rem / OW, ow = rem - rr * OW;
        const int oh = oh0 + rr;
        st[j] = (ci < CHK && oh >= 0 && oh < OH) ? (ci << 24) | (oh * ps_h + ow) : -1;
    }
    // ---- the pixel's pooling windows (k = 3, s = 2): rows oh = py>>1 (a = 0) and oh - 1 (a = 1), columns ow = px>>1 (b = 0)
    // and ow - 1 (b = 1).  Addresses: entry (row, ow - 1) of slab 0, +1 entry for b = 0; wloc = the window-local index the
    // arg-max byte must equal for the window to route its gradient to this pixel (254 = never).
    int wloc[4];
    uint32_t rowaddr[2];
#pragma unroll
    for (int a = 0; a < 2; ++a) {
        const int oh = (py >> 1) - a, lr = (py & 1) + 2 * a;
        const bool rok = valid && oh >= 0 && oh < OH && lr <= 2;
#pragma unroll
        for (int b = 0; b < 2; ++b) {
            const int ow = (px >> 1) - b, lc = (px & 1) + 2 * b;
            wloc[a * 2 + b] = (rok && ow >= 0 && ow < OW && lc <= 2) ? lr * 3 + lc : 254;
        }
        const int rr = min(max(oh - oh0, 0), prow - 1);               // clamped: unreachable windows still read inside the buffer
        rowaddr[a] = (uint32_t)(8 + rr * OW + (px >> 1) - 1) * 8u;    // byte offset in a buffer; entry 8 = slab 0, row 0, column 0
    }
    const uint32_t slab_bytes = (uint32_t)rowlen * 8u;

    const __amdgpu_buffer_rsrc_t rs_x = C8 == 2 ? pw_rsrc(reinterpret_cast<const char*>(x) + (int64_t)img * ((C + 7) / 8) * HW * 16,
                                                          (int64_t)((C + 7) / 8) * HW * 16)
                                                : pw_rsrc(x + (int64_t)img * C * HW, (int64_t)C * HW * 4);
    const int wp = W + 2 * halo;
    const int dplane = (H + 2 * halo) * wp;
    static_assert(C8 == 0 || CHK == 8, "packed output: 8-channel chunks");
    const int CB = (C + 7) / 8;
    const __amdgpu_buffer_rsrc_t rs_dx = C8 ? pw_rsrc(reinterpret_cast<const char*>(dx) + (int64_t)img * CB * dplane * 16, (int64_t)CB * dplane * 16)
                                            : pw_rsrc(dx + (int64_t)img * C * dplane, (int64_t)C * dplane * 4);
    const __amdgpu_buffer_rsrc_t rs_dp = pw_rsrc(dp + (int64_t)img * ps_n, pooled_bytes_f);
    const __amdgpu_buffer_rsrc_t rs_arg = pw_rsrc(arg + (int64_t)img * ps_n, pooled_bytes_f / 4);
    const uint32_t voff_x = valid ? (uint32_t)(py * W + px) * (C8 == 2 ? 16u : 4u) : PW_OOB;
    const uint32_t voff_dx = C8 == 0 ? (inplane ? (uint32_t)((py + halo) * wp + pxq) * 4u : PW_OOB)
                                     : (valid ? (uint32_t)((py + halo) * wp + px + halo) * 16u : PW_OOB);
    const int x_cs = HW * 4, dx_cs = dplane * 4;                      // channel strides in bytes

    float dpv[NST];
    uint32_t av[NST];
    auto stage_load = [&](int c0) {                                   // slab ci holds channel c0 - 2 + ci
#pragma unroll
        for (int j = 0; j < NST; ++j) {
            const int c = c0 - 2 + (st[j] >> 24);
            const bool ok = st[j] >= 0 && c >= 0 && c < C;
            const int off = c * ps_c + (st[j] & 0xffffff);
            dpv[j] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rs_dp, ok ? off * 4 : (int)PW_OOB, 0, 0));
            av[j] = (uint32_t)__builtin_amdgcn_raw_buffer_load_b8(rs_arg, ok ? off : (int)PW_OOB, 0, 0);
        }
    };
    auto stage_write = [&](int buf) {
#pragma unroll
        for (int j = 0; j < NST; ++j) stage[buf * BUF + 8 + threadIdx.x + 256 * j] = make_uint2(__builtin_bit_cast(uint32_t, dpv[j]), av[j]);
    };
    float xa[CHK], xb[CHK];
    auto x_load = [&](int c0, float (&v)[CHK]) {
        if constexpr (C8 == 2) {                                      // c0 is a multiple of 8: one chunk; blocks past C answer 0
            typedef uint32_t u4 __attribute__((ext_vector_type(4)));
            const u4 w = __builtin_bit_cast(u4, __builtin_amdgcn_raw_buffer_load_b128(rs_x, (int)(c0 < C ? voff_x : PW_OOB), (c0 >> 3) * HW * 16, 0));
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                v[2 * i] = __uint_as_float(w[i] << 16);
                v[2 * i + 1] = __uint_as_float(w[i] & 0xffff0000u);
            }
        } else {
#pragma unroll
            for (int i = 0; i < CHK; ++i) {
                const int cc = c0 + i;                                    // uniform; channels past C: the range check answers 0
                v[i] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rs_x, (int)(cc >= 0 && cc < C ? voff_x : PW_OOB), max(cc, 0) * x_cs, 0));
            }
        }
    };

    float xw0 = 0.f, xw1 = 0.f, xw2 = 0.f, xw3 = 0.f, xw4 = 0.f;      // x[cc-4 .. cc]
    float tw0 = 0.f, tw1 = 0.f, tw2 = 0.f, tw3 = 0.f, tw4 = 0.f;      // t[cc-6 .. cc-2]
    float uw0 = 0.f, uw1 = 0.f, uw2 = 0.f;                            // u[cc-4 .. cc-2]
    const float k2ab = 2.f * alpha * 0.75f;
    const unsigned char* sbytes = reinterpret_cast<const unsigned char*>(stage);

    // one chunk: no branch inside, so the LDS reads and the math of neighbouring channels interleave freely
    auto chunk = [&](int c0, int buf, const float (&xin)[CHK]) {
        const uint32_t b0 = (uint32_t)(buf * BUF) * 8u;
        uint32_t a0 = b0 + rowaddr[0], a1 = b0 + rowaddr[1];
        float rr[4];
#pragma unroll
        for (int i = 0; i < CHK; ++i) {
            const int cc = c0 + i;
            // routed pooling gradient of channel cc - 2 (slab i)
            const uint2 e00 = *reinterpret_cast<const uint2*>(sbytes + a0 + 8), e01 = *reinterpret_cast<const uint2*>(sbytes + a0);
            const uint2 e10 = *reinterpret_cast<const uint2*>(sbytes + a1 + 8), e11 = *reinterpret_cast<const uint2*>(sbytes + a1);
            a0 += slab_bytes;
            a1 += slab_bytes;
            float g = 0.f;
            g += ((int)e00.y == wloc[0]) ? __builtin_bit_cast(float, e00.x) : 0.f;
            g += ((int)e01.y == wloc[1]) ? __builtin_bit_cast(float, e01.x) : 0.f;
            g += ((int)e10.y == wloc[2]) ? __builtin_bit_cast(float, e10.x) : 0.f;
            g += ((int)e11.y == wloc[3]) ? __builtin_bit_cast(float, e11.x) : 0.f;
            xw0 = xw1; xw1 = xw2; xw2 = xw3; xw3 = xw4; xw4 = xin[i];
            float s = 0.f;
            s += xw0 * xw0; s += xw1 * xw1; s += xw2 * xw2; s += xw3 * xw3; s += xw4 * xw4;
            const float sc = bias + alpha * s;
            const float rq = __builtin_amdgcn_rsqf(sc);
            const float pw = rq * __builtin_amdgcn_sqrtf(rq);        // sc^-0.75 (pow_neg's beta = 0.75 form)
            tw0 = tw1; tw1 = tw2; tw2 = tw3; tw3 = tw4;
            tw4 = g * xw2 * pw * (rq * rq);                           // sc^-1 = (sc^-1/2)^2: a multiply instead of a third quarter-rate op
            uw0 = uw1; uw1 = uw2; uw2 = g * pw;
            const int oc = cc - 4;                                    // uniform; outside [0, C): the store's range check drops it
            float a = 0.f;
            a += tw0; a += tw1; a += tw2; a += tw3; a += tw4;
            float r = uw0 - k2ab * xw0 * a;
            if (RELU) r = xw0 > 0.f ? r : 0.f;
            if constexpr (C8 != 0) {
                rr[i & 3] = r;
                if ((i & 3) == 3) {                                   // channels oc - 3 .. oc: half a chunk of block (oc - 3) >> 3
                    typedef float f2 __attribute__((ext_vector_type(2)));
                    typedef __bf16 b2 __attribute__((ext_vector_type(2)));
                    typedef uint32_t u2 __attribute__((ext_vector_type(2)));
                    const u2 w = {__builtin_bit_cast(uint32_t, __builtin_convertvector(f2{rr[0], rr[1]}, b2)),
                                  __builtin_bit_cast(uint32_t, __builtin_convertvector(f2{rr[2], rr[3]}, b2))};
                    const int blk = (oc - 3) >> 3;                    // uniform; outside [0, CB): dropped by the range check
                    // (round 4, measured and dropped: holding the lower half of a chunk in registers and storing the whole 16-byte chunk
                    // at once -- 0.54 -> 0.75 ms on layer 1)
                    __builtin_amdgcn_raw_buffer_store_b64(w, rs_dx, (int)((oc - 3 >= R0 && oc - 3 < R1 && blk < CB) ? voff_dx + (((oc - 3) & 7) * 2) : PW_OOB),
                                                          blk * dplane * 16, 0);
                }
            } else {
                __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(uint32_t, r), rs_dx, (int)((oc >= R0 && oc < R1) ? voff_dx : PW_OOB),
                                                      oc * dx_cs, 0);
            }
        }
    };

    const int nchunks = (R1 + 4 - cs + CHK - 1) / CHK;
    // The pad entries of both buffers (8 in front: "entry -1" of a band's first pooled row; 8 behind) are READ by pixels whose window
    // does not exist and rejected only by their arg-max word never equalling wloc = 254 -- so they must not hold stale LDS bytes:
    // beside a kernel that leaves 0xfe words in LDS (the split-bf16 wgrad on a second stream) one step in three had ~170 of 67 M
    // gradient elements pick up a stale "dp" (round 3).  {0, 255} matches no window.
    if (threadIdx.x < 32) {
        const int t = threadIdx.x & 15, b2 = threadIdx.x >> 4;
        stage[b2 * BUF + (t < 8 ? t : NST * 256 + t)] = make_uint2(0u, 255u);
    }
    stage_load(cs);
    x_load(cs, xa);
    stage_write(0);
    __syncthreads();
    for (int k = 0; k < nchunks; k += 2) {                            // unrolled by two: the x registers alternate without copies
        stage_load(cs + (k + 1) * CHK);                               // next chunk's traffic goes out before this chunk's math;
        x_load(cs + (k + 1) * CHK, xb);                               // past the last channel every lane fails the channel test
        chunk(cs + k * CHK, 0, xa);
        stage_write(1);
        __syncthreads();
        if (k + 1 >= nchunks) break;
        stage_load(cs + (k + 2) * CHK);
        x_load(cs + (k + 2) * CHK, xa);
        chunk(cs + (k + 1) * CHK, 1, xb);
        stage_write(0);
        __syncthreads();
    }
}

// Channel ranges per (band, image) of the channel-stream backward: the count (<= 4) with the fewest rounds x channels walked, a
// round = 8 workgroups per CU (56 VGPRs, 12.5 KB of LDS).  `unit`: ranges start at multiples of it (8 for the packed output).
static int g_plb_forced_ranges = 0;
static int g_lpf_forced_ranges = 0;            // tests: vl_pool_lrn_bwd_test_ranges forces the forward's channel-range count as well
static int plb_channel_ranges(int64_t workgroups, int c, int unit, int lead, int* cper) {
    const int64_t slots = 8ll * vl_device_cus();
    int best = 1;
    int64_t best_cost = 0;
    for (int sp = 1; sp <= 4; ++sp) {
        const int per = (int)(((c + sp - 1) / sp + unit - 1) / unit * unit);
        if (sp > 1 && (per * (sp - 1) >= c || per < lead)) continue;  // the last range would be empty / a range shorter than the lead-in
        const int64_t cost = ((workgroups * sp + slots - 1) / slots) * (per + 12);
        if (sp == 1 || cost < best_cost) { best = sp; best_cost = cost; *cper = per; }
    }
    if (g_plb_forced_ranges >= 1 && g_plb_forced_ranges <= 4) {            // tests: vl_pool_lrn_bwd_test_ranges
        best = g_plb_forced_ranges;
        *cper = (int)(((c + best - 1) / best + unit - 1) / unit * unit);
        while (best > 1 && (*cper * (best - 1) >= c || *cper < lead)) {   // a range must start >= `lead` channels in (the kernel's walk
            --best;                                                        // restarts that far below its first output channel)
            *cper = (int)(((c + best - 1) / best + unit - 1) / unit * unit);
        }
    }
    return best;
}

/* Test hook (not part of the operator surface): force the number of channel ranges per (band, image) of vl_pool_lrn_bwd /
 * vl_pool_lrn_bwd_c8 to 1..4 (fewer when the channel count does not allow it); 0 = the cost model.  Process-wide, not thread-safe. */
extern "C" int vl_pool_lrn_bwd_test_ranges(int ranges) {
    VL_CHECK(ranges >= 0 && ranges <= 4, "vl_pool_lrn_bwd_test_ranges: 0 (automatic) .. 4");
    g_plb_forced_ranges = ranges;
    g_lpf_forced_ranges = ranges;                 // vl_lrn_pool_fwd / _c8 split their channel walk the same way (at most 8 ranges on their own)
    return 0;
}

extern "C" int vl_pool_lrn_bwd(const float* x, const float* dp, const uint8_t* argmax, float* dx, int n, int c, int h, int w,
                               int p_halo, int radius, float alpha, float beta, float bias, int relu_fused, int dx_halo,
                               vl_stream_t stream) {
    VL_CHECK(x && dp && argmax && dx && n > 0 && c > 0 && h >= 3 && w >= 3 && p_halo >= 0 && dx_halo >= 0, "vl_pool_lrn_bwd: bad argument");
    VL_CHECK(radius == 2, "vl_pool_lrn_bwd: only depth_radius 2 is built (alexnet.py:81); got %d", radius);
    const int oh = (h - 3) / 2 + 1, ow = (w - 3) / 2 + 1;
    const int owp = ow + 2 * p_halo;
    const int64_t pplane = (int64_t)(oh + 2 * p_halo) * owp;
    const int64_t origin = (int64_t)p_halo * owp + p_halo;
    VL_CHECK(n <= 65528, "vl_pool_lrn_bwd: batch %d exceeds the grid limit", n);
    {   // channel-stream form: a 256-pixel band x one channel chunk of pooled entries must fit NST * 256 staging slots
        const int rows = (255 + w - 1) / w + 1;                        // input rows a 256-pixel band can touch
        const int max_prow = rows / 2 + 2;
        const int64_t bytes_x = (int64_t)(c + 24) * h * w * 4, bytes_dx = (int64_t)(c + 24) * (h + 2 * dx_halo) * (w + 2 * dx_halo) * 4;
        const int64_t pooled_f = ((int64_t)c * pplane - origin) * 4;
        const bool ok = beta == 0.75f && bytes_x < (1ll << 31) && bytes_dx < (1ll << 31) && pooled_f < (1ll << 31) && pplane < (1 << 24) &&
                        !kPoolLrnChunked;
        int cper = c;
        const int nz = plb_channel_ranges((int64_t)ceil_div((int64_t)h * (w + 2 * dx_halo), 256) * n, c, 1, 4, &cper);
        const dim3 grid(ceil_div((int64_t)h * (w + 2 * dx_halo), 256), (n + 7) / 8 * 8, nz);   // bands over halo-layout rows; images padded to the 8 XCDs
        const int64_t psn = (int64_t)c * pplane;
#define VL_PLB_LAUNCH(CHK, NST)                                                                                                     \
    do {                                                                                                                            \
        if (relu_fused)                                                                                                             \
            hipLaunchKernelGGL((pool_lrn_bwd_stream_kernel<CHK, NST, true, 0>), grid, dim3(256), 0, (hipStream_t)stream, x, dp + origin, \
                               argmax + origin, dx, c, h, w, oh, ow, psn, (int)pplane, owp, pooled_f, alpha, bias, dx_halo, cper, n);  \
        else                                                                                                                        \
            hipLaunchKernelGGL((pool_lrn_bwd_stream_kernel<CHK, NST, false, 0>), grid, dim3(256), 0, (hipStream_t)stream, x, dp + origin, \
                               argmax + origin, dx, c, h, w, oh, ow, psn, (int)pplane, owp, pooled_f, alpha, bias, dx_halo, cper, n);  \
        VL_LAUNCH_CHECK();                                                                                                          \
        return 0;                                                                                                                   \
    } while (0)
        // chunk = 5 channels (110 registers, 12.5 KB of LDS: four workgroups per CU instead of two) when C + 4 is a multiple of it (96
        // and 256 are: no idle tail iterations): layer 1 0.79 -> 0.71 ms, layer 2 0.57 -> 0.51 ms against the 20-channel chunks of
        // round 1 (VL_POOL_LRN_BWD_R1=1)
        static const bool r1 = vl_exp_env("VL_POOL_LRN_BWD_R1") != nullptr;
        if (ok && !r1 && (c + 4) % 5 == 0 && (int64_t)5 * max_prow * ow <= 3 * 256) VL_PLB_LAUNCH(5, 3);
        // chunk = 20 channels when C + 4 is a multiple of it (96 and 256 are): no idle tail iterations
        if (ok && (c + 4) % 20 == 0 && (int64_t)20 * max_prow * ow <= 11 * 256 && !kPoolLrnChk16) VL_PLB_LAUNCH(20, 11);
        if (ok && (int64_t)16 * max_prow * ow <= 9 * 256) VL_PLB_LAUNCH(16, 9);
#undef VL_PLB_LAUNCH
    }
    constexpr int CH = 16, NPIX = 512;
    const int max_prow = ((NPIX + w - 1) / w + 1) / 2 + 3;             // pooled rows one band can touch
    const size_t lds = (((size_t)(CH + 4) * max_prow * ow * (sizeof(float) + 1)) + 15) & ~(size_t)15;
    VL_CHECK(lds <= 64 * 1024, "vl_pool_lrn_bwd: pooled plane too wide (%d) for the LDS staging", ow);
    dim3 grid(ceil_div((int64_t)h * w, NPIX), ceil_div(c, CH), n);
    hipLaunchKernelGGL((pool_lrn_bwd_kernel<CH, 2, NPIX>), grid, dim3(256), lds, (hipStream_t)stream, x, dp + origin, argmax + origin, dx,
                       c, h, w, oh, ow, (int64_t)c * pplane, (int)pplane, owp, alpha, beta, bias, relu_fused, dx_halo);
    VL_LAUNCH_CHECK();
    return 0;
}

/* vl_pool_lrn_bwd writing the packed-bf16 gradient dxb ("c8" layout of conv_c8.hip, dxb_halo) instead of fp32 dx: what the bf16 conv
 * path's wgrad / dgrad / bias gradient read.  Channel-stream form only (beta 0.75, planes that fit its staging). */
extern "C" int vl_pool_lrn_bwd_c8(const void* x, int x_packed, const float* dp, const uint8_t* argmax, void* dxb, int n, int c, int h, int w,
                                  int p_halo, int radius, float alpha, float beta, float bias, int relu_fused, int dxb_halo, vl_stream_t stream) {
    VL_CHECK(x && dp && argmax && dxb && n > 0 && c > 0 && h >= 3 && w >= 3 && p_halo >= 0 && dxb_halo >= 0, "vl_pool_lrn_bwd_c8: bad argument");
    VL_CHECK(radius == 2 && beta == 0.75f, "vl_pool_lrn_bwd_c8: only depth_radius 2, beta 0.75 are built (alexnet.py:81-84)");
    VL_CHECK(n <= 65528, "vl_pool_lrn_bwd_c8: batch %d exceeds the grid limit", n);
    const int oh = (h - 3) / 2 + 1, ow = (w - 3) / 2 + 1;
    const int owp = ow + 2 * p_halo;
    const int64_t pplane = (int64_t)(oh + 2 * p_halo) * owp;
    const int64_t origin = (int64_t)p_halo * owp + p_halo;
    const int rows = (255 + w - 1) / w + 1, max_prow = rows / 2 + 2;
    const int64_t bytes_x = (int64_t)(c + 24) * h * w * 4, bytes_dx = (int64_t)((c + 7) / 8 + 3) * (h + 2 * dxb_halo) * (w + 2 * dxb_halo) * 16;
    const int64_t pooled_f = ((int64_t)c * pplane - origin) * 4;
    VL_CHECK(bytes_x < (1ll << 31) && bytes_dx < (1ll << 31) && pooled_f < (1ll << 31) && pplane < (1 << 24) && (int64_t)8 * max_prow * ow <= 5 * 256,
             "vl_pool_lrn_bwd_c8: plane too large for the channel-stream form");
    int cper = c;
    const int nz = plb_channel_ranges((int64_t)ceil_div((int64_t)h * w, 256) * n, c, 8, 8, &cper);
    const dim3 grid(ceil_div((int64_t)h * w, 256), (n + 7) / 8 * 8, nz);
    const int64_t psn = (int64_t)c * pplane;
    const float* xf = (const float*)x;
#define VL_PLBC(RELU, MODE)                                                                                                             \
    hipLaunchKernelGGL((pool_lrn_bwd_stream_kernel<8, 5, RELU, MODE>), grid, dim3(256), 0, (hipStream_t)stream, xf, dp + origin, argmax + origin, \
                       (float*)dxb, c, h, w, oh, ow, psn, (int)pplane, owp, pooled_f, alpha, bias, dxb_halo, cper, n)
    if (relu_fused && x_packed) VL_PLBC(true, 2);
    else if (relu_fused) VL_PLBC(true, 1);
    else if (x_packed) VL_PLBC(false, 2);
    else VL_PLBC(false, 1);
#undef VL_PLBC
    VL_LAUNCH_CHECK();
    return 0;
}

extern "C" int vl_lrn_fwd(const float* x, float* y, int n, int c, int hw, int radius, float alpha, float beta, float bias,
                          vl_stream_t stream) {
    VL_CHECK(x && y && n > 0 && c > 0 && hw > 0, "vl_lrn_fwd: bad argument");
    VL_CHECK(radius == 2, "vl_lrn_fwd: only depth_radius 2 is built (alexnet.py:81); got %d", radius);
    constexpr int CH = 32;
    dim3 grid(ceil_div((int64_t)n * hw, 256), ceil_div(c, CH));
    hipLaunchKernelGGL((lrn_fwd_kernel<CH, 2>), grid, dim3(256), 0, (hipStream_t)stream, x, y, n, c, hw, alpha, beta, bias);
    VL_LAUNCH_CHECK();
    return 0;
}

extern "C" int vl_lrn_bwd(const float* x, const float* dy, float* dx, int n, int c, int hw, int radius, float alpha, float beta,
                          float bias, int relu_fused, int w, int dx_halo, vl_stream_t stream) {
    VL_CHECK(x && dy && dx && n > 0 && c > 0 && hw > 0, "vl_lrn_bwd: bad argument");
    VL_CHECK(w > 0 && hw % w == 0 && dx_halo >= 0, "vl_lrn_bwd: plane width %d does not divide hw %d", w, hw);
    VL_CHECK(radius == 2, "vl_lrn_bwd: only depth_radius 2 is built (alexnet.py:81); got %d", radius);
    constexpr int CH = 16;
    dim3 grid(ceil_div((int64_t)n * hw, 256), ceil_div(c, CH));
    hipLaunchKernelGGL((lrn_bwd_kernel<CH, 2>), grid, dim3(256), 0, (hipStream_t)stream, x, dy, dx, n, c, hw, alpha, beta, bias,
                       relu_fused, w, dx_halo);
    VL_LAUNCH_CHECK();
    return 0;
}

// ---- fused forward of [LRN -> max_pool 3x3/2 VALID] (alexnet.py:79-98, 120-139) -------------------------------------
// The LRN output is only ever the pool's input (the backward pass reads the LRN INPUT, vl_pool_lrn_bwd), so it is never
// written to HBM: lrn1 + pool1 moved 2 x 1.28 + 1.28 + 0.39 GB per step through two kernels; fused it is 1.28 + 0.39 GB.
// One workgroup = one image x a band of PRB pooled rows (= 2 PRB + 1 input rows); a thread owns PPT pixels of the band and
// walks ALL channels with the 5-wide LRN window in registers (channel cc enters at iteration cc, LRN output cc - 2 leaves),
// the next chunk's loads in flight behind the current chunk's math.  Each chunk of CHK LRN outputs goes to LDS (two buffers,
// one barrier per chunk); the chunk's pooled outputs (<= NSL per thread, their window origins decoded once) take the
// strict-> first maximum of 9 LDS reads, exactly vl_maxpool_fwd's scan order, and are stored in the pool-output halo layout.
// C8: pout is the packed-bf16 "c8" tensor [image][C / 8][pooled plane][8] (conv_c8.hip) instead of fp32 NCHW: each pooled output is
// stored as one bf16 (nearest even) at its channel's slot of the pixel's chunk; the arg-max map is unchanged.
// C8 == 2: x is packed too ([image][C / 8][H][W][8] bf16, no halo): a 16-byte load per pixel brings 8 channels = four 2-channel chunks.
template <int CHK, int PPT, int NSL, int C8 = 0>
__global__ __launch_bounds__(512) void lrn_pool_fwd_kernel(const float* __restrict__ x, float* __restrict__ pout,
                                                           uint8_t* __restrict__ argout, int C, int H, int W, int OH, int OW, int prb,
                                                           int pplane, int owp, int p_halo, float alpha, float bias, int cper, int nimg) {
    extern __shared__ __attribute__((aligned(16))) float lbuf[];      // [2][CHK][npix]
    // blockIdx.z owns the OUTPUT channels [R0, R1) (cper of them, a multiple of CHK; the whole tensor when the grid is flat): its walk
    // starts two channels (one chunk) early so that the LRN window of channel R0 is complete, and ends two channels late.  Few-frame
    // launches only (round 4): 128 frames of layer 2 were 512 two-wave workgroups walking 256 channels each, 79 us where 1/8 of the
    // 1024-frame time is 37.
    const int R0 = blockIdx.z * cper, R1 = min(C, R0 + cper);
    const int cs = max(R0 - CHK, 0);                                  // CHK >= 2 = the LRN radius
    const int T = blockDim.x;
    int band, img;
    if (!xcd_band_image(nimg, band, img)) return;                     // bands of an image share an input row at every seam
    const int oh_a = band * prb;
    const int nprow = min(prb, OH - oh_a);                            // pooled rows of this band
    const int npix = (2 * nprow + 1) * W;                             // input pixels of this band
    const int p_base = 2 * oh_a * W;
    const int HW = H * W;
    const int CB = (C + 7) / 8;
    const __amdgpu_buffer_rsrc_t rs_x = C8 == 2 ? pw_rsrc(reinterpret_cast<const char*>(x) + (int64_t)img * CB * HW * 16, (int64_t)CB * HW * 16)
                                                : pw_rsrc(x + (int64_t)img * C * HW, (int64_t)C * HW * 4);
    const __amdgpu_buffer_rsrc_t rs_p = C8 != 0 ? pw_rsrc(reinterpret_cast<const char*>(pout) + (int64_t)img * CB * pplane * 16, (int64_t)CB * pplane * 16)
                                           : pw_rsrc(pout + (int64_t)img * C * pplane, (int64_t)C * pplane * 4);
    const __amdgpu_buffer_rsrc_t rs_a = pw_rsrc(argout + (int64_t)img * C * pplane, (int64_t)C * pplane);
    uint32_t voff_x[PPT];
    int lpix[PPT];                                                    // band-local pixel, -1 = none
#pragma unroll
    for (int q = 0; q < PPT; ++q) {
        const int pix = threadIdx.x + q * T;
        lpix[q] = pix < npix ? pix : -1;                              // (-1: its LRN values go to the buffer's spare slot)
        voff_x[q] = pix < npix ? (uint32_t)(p_base + pix) * (C8 == 2 ? 16u : 4u) : PW_OOB;
    }
    // pooled outputs of a chunk: o = tid + s T  <->  (slab ci, pooled row, pooled column)
    // fp32 output: the slots enumerate WHOLE rows of the halo layout, halo columns included (they store 0.0 = what the halo holds by
    // contract; the arg-max map's halo is never read), so that a wave's stores are runs of full 32-byte sectors.  Round 4, parts of the
    // kernel compiled out (VL_LRN_POOL_FORM, experiment build): loads + LRN + LDS writes alone ran at 5.4 - 5.9 TB/s, the two stores per
    // pooled output -- 112-byte value rows and 28-byte arg-max rows at a 128- / 32-byte pitch: every sector of the arg-max map written
    // partially -- cost a third of the kernel.  The packed output (C8) keeps interior slots (2-byte stores into 16-byte chunks).
    constexpr bool ROWS = C8 == 0;
    int s_lds[NSL], s_out[NSL];                                       // LDS float offset of the window origin | ci << 24 | output element offset
    uint32_t s_halo = 0;                                              // bit sl: slot sl is a halo column (stores 0)
    const int row_w = ROWS ? owp : OW;
    const int per_slab = nprow * row_w;
#pragma unroll
    for (int sl = 0; sl < NSL; ++sl) {
        const int o = threadIdx.x + sl * T;
        const int ci = o / per_slab, rem = o - ci * per_slab;
        const int ohl = rem / row_w, col = rem - ohl * row_w;
        const int ow = ROWS ? col - p_halo : col;
        const bool ok = ci < CHK;
        const bool inner = ow >= 0 && ow < OW;
        s_lds[sl] = (ok && inner) ? ci * npix + 2 * ohl * W + 2 * ow : 0;
        s_out[sl] = ok ? (ci << 24) | ((oh_a + ohl + p_halo) * owp + ow + p_halo) : -1;
        if (ok && !inner) s_halo |= 1u << sl;
    }
    const int x_cs = HW * 4;
    float xa[PPT][CHK], xb[PPT][CHK];
    auto x_load = [&](int c0, float (&v)[PPT][CHK]) {
#pragma unroll
        for (int i = 0; i < CHK; ++i) {
            const int cc = c0 + i;                                    // uniform; channels past C: the range check answers 0
#pragma unroll
            for (int q = 0; q < PPT; ++q)
                v[q][i] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rs_x, (int)(cc < C ? voff_x[q] : PW_OOB), cc * x_cs, 0));
        }
    };
    float xw[PPT][5];
#pragma unroll
    for (int q = 0; q < PPT; ++q)
#pragma unroll
        for (int d = 0; d < 5; ++d) xw[q][d] = 0.f;

    auto chunk = [&](int c0, int buf, const float (&xin)[PPT][CHK]) {
        float* lb = lbuf + buf * (CHK * npix + 1);                    // + 1: the spare slot idle lanes write to (no exec-mask branch)
        // LRN outputs of channels c0 - 2 .. c0 + CHK - 3 -> slabs 0 .. CHK - 1
#pragma unroll
        for (int i = 0; i < CHK; ++i) {
#pragma unroll
            for (int q = 0; q < PPT; ++q) {
                xw[q][0] = xw[q][1]; xw[q][1] = xw[q][2]; xw[q][2] = xw[q][3]; xw[q][3] = xw[q][4]; xw[q][4] = xin[q][i];
                float sq = 0.f;
#pragma unroll
                for (int d = 0; d < 5; ++d) sq += xw[q][d] * xw[q][d];
                const float sc = bias + alpha * sq;
                const float rq = __builtin_amdgcn_rsqf(sc);
                const float l = xw[q][2] * (rq * __builtin_amdgcn_sqrtf(rq));   // x * sc^-0.75 (pow_neg's beta = 0.75 form)
                lb[lpix[q] >= 0 ? i * npix + lpix[q] : CHK * npix] = l;
            }
        }
        __syncthreads();
#pragma unroll
        for (int sl = 0; sl < NSL; ++sl) {
            const int c = c0 - 2 + (s_out[sl] >> 24);
            const bool live = s_out[sl] >= 0 && c >= R0 && c < R1;    // dead lanes scan slab 0's first window and store out of range
            {
                const float* wp = lb + s_lds[sl];
                float best = -INFINITY;
                int bi = 0;
#pragma unroll
                for (int i = 0; i < 3; ++i)
#pragma unroll
                    for (int j = 0; j < 3; ++j) {
                        const float v = wp[i * W + j];
                        if (v > best) {                               // strict: the first maximum in scan order wins
                            best = v;
                            bi = i * 3 + j;
                        }
                    }
                const int off = c * pplane + (s_out[sl] & 0xffffff);
                if (ROWS && ((s_halo >> sl) & 1u)) {                  // halo column: dead lanes scanned slab 0's first window
                    best = 0.f;
                    bi = 0;
                }
                if constexpr (C8 != 0) {
                    // (round 4, measured and dropped: gathering a pixel's 8-channel block in registers and storing it as ONE 16-byte
                    // word -- the pooling phase then runs on half the threads with two windows each and the kernel got 10 % slower)
                    const __bf16 hb = (__bf16)best;
                    __builtin_amdgcn_raw_buffer_store_b16(__builtin_bit_cast(uint16_t, hb), rs_p,
                                                          live ? ((c >> 3) * pplane + (s_out[sl] & 0xffffff)) * 16 + (c & 7) * 2 : (int)PW_OOB, 0, 0);
                } else {
                    __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(uint32_t, best), rs_p, live ? off * 4 : (int)PW_OOB, 0, 0);
                }
                __builtin_amdgcn_raw_buffer_store_b8((uint8_t)bi, rs_a, live ? off : (int)PW_OOB, 0, 0);
            }
        }
    };
    const int nchunks = (R1 + 2 - cs + CHK - 1) / CHK;
    if constexpr (C8 == 2) {
        static_assert(C8 != 2 || CHK == 2, "packed input: 2-channel chunks (one dword of a pixel's 16-byte block)");
        typedef uint32_t u4 __attribute__((ext_vector_type(4)));
        u4 cur[PPT], nxt[PPT];
        auto blk_load = [&](int kb, u4 (&v)[PPT]) {                   // channels 8 kb .. 8 kb + 7; blocks past C answer 0
#pragma unroll
            for (int q = 0; q < PPT; ++q)
                v[q] = __builtin_bit_cast(u4, __builtin_amdgcn_raw_buffer_load_b128(rs_x, (int)(kb < CB ? voff_x[q] : PW_OOB), kb * HW * 16, 0));
        };
        // (channel ranges of the packed form are multiples of 8: cs = R0 - 2 lies in the block before R0's; the walk starts at that
        // block's first chunk and the chunks below cs only fill the window -- they compute channels the `live` test drops)
        const int kb0 = cs >> 3, kend = (R1 + 2 + CHK - 1) / CHK;     // first block; chunk index (from channel 0) behind the last one
        blk_load(kb0, cur);
        for (int kb = kb0; kb * 4 < kend; ++kb) {
            blk_load(kb + 1, nxt);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                if (kb * 4 + j >= kend) break;
                float xin[PPT][CHK];
#pragma unroll
                for (int q = 0; q < PPT; ++q) {
                    xin[q][0] = __uint_as_float(cur[q][j] << 16);
                    xin[q][1] = __uint_as_float(cur[q][j] & 0xffff0000u);
                }
                chunk((kb * 4 + j) * CHK, j & 1, xin);
            }
#pragma unroll
            for (int q = 0; q < PPT; ++q) cur[q] = nxt[q];
        }
        return;
    }
    x_load(cs, xa);
    for (int k = 0; k < nchunks; k += 2) {                            // unrolled by two: the x registers alternate without copies
        x_load(cs + (k + 1) * CHK, xb);
        chunk(cs + k * CHK, 0, xa);
        if (k + 1 >= nchunks) break;
        x_load(cs + (k + 2) * CHK, xa);
        chunk(cs + (k + 1) * CHK, 1, xb);
    }
}

template <int CHK, int PPT, int NSL, int C8 = 0>
static int launch_lrn_pool_fwd(const float* x, float* p, uint8_t* argmax, int n, int c, int h, int w, int p_halo, float alpha, float bias,
                               hipStream_t stream) {
    const int oh = (h - 3) / 2 + 1, ow = (w - 3) / 2 + 1;
    const int owp = ow + 2 * p_halo;
    const int64_t pplane = (int64_t)(oh + 2 * p_halo) * owp;
    // band = prb pooled rows: the largest that fits PPT pixels per thread of a <= 512-thread workgroup, NSL outputs per thread
    // and 64 KB of LDS; then the smallest thread count (multiple of 64) that still covers it
    int prb = 0, threads = 0;
    for (int cand = oh; cand >= 1 && !prb; --cand) {
        const int npix = (2 * cand + 1) * w;
        const int need_px = ceil_div(npix, PPT), need_out = ceil_div((int64_t)CHK * cand * (C8 == 0 ? owp : ow), NSL);
        int t = ceil_div(need_px > need_out ? need_px : need_out, 64) * 64;
        if (t <= 512 && (size_t)2 * (CHK * npix + 1) * sizeof(float) <= 64 * 1024) {
            prb = cand;
            threads = t < 64 ? 64 : t;
        }
    }
    VL_CHECK(prb > 0, "vl_lrn_pool_fwd: plane too wide (%d) for one band of pooled rows", w);
    // balance the bands (e.g. 28 pooled rows, at most 5 per band -> 6 bands of 5,5,5,5,4,4 rather than 5,5,5,5,5,3); few frames (one
    // rank's 128-frame shard of the 8-GPU job: layer 2 was ONE band x 128 images = half the CUs, 98 us where 1/8 of the 1024-frame time
    // is 37): cut more bands, up to two workgroups per CU, at the price of their shared input rows (round 4)
    int bands = ceil_div(oh, prb);
    const int want = ceil_div(2 * (int64_t)vl_device_cus(), n);
    if (bands < want) bands = want < oh ? want : oh;
    prb = ceil_div(oh, bands);
    bands = ceil_div(oh, prb);
    {
        const int need_px = ceil_div((2 * prb + 1) * w, PPT), need_out = ceil_div((int64_t)CHK * prb * (C8 == 0 ? owp : ow), NSL);
        threads = ceil_div(need_px > need_out ? need_px : need_out, 64) * 64;
    }
    const size_t lds = (size_t)2 * (CHK * (2 * prb + 1) * w + 1) * sizeof(float);       // two buffers, each with a spare slot
    static const bool verbose = vl_exp_env("VL_LRN_POOL_VERBOSE") != nullptr;
    if (verbose) fprintf(stderr, "lrn_pool_fwd<%d,%d,%d>: bands %d prb %d threads %d lds %zu\n", CHK, PPT, NSL, bands, prb, threads, lds);
    // channel ranges (grid z) until the launch holds eight workgroups per CU, in units of 8 channels (whole packed blocks, whole chunks),
    // at least 32 channels each: every range re-reads 2 + 2 channels of its neighbours
    int nz = 1, cper = c;
    {
        const int64_t wgs = (int64_t)bands * n, slots = 8ll * vl_device_cus();
        const int can = c / 32 > 0 ? c / 32 : 1;
        int wantz = (int)((slots + wgs - 1) / wgs);
        wantz = wantz > 8 ? 8 : wantz;
        wantz = wantz > can ? can : wantz;
        if (g_lpf_forced_ranges >= 1) wantz = g_lpf_forced_ranges;
        if (wantz > 1) {
            cper = ((c + wantz - 1) / wantz + 7) / 8 * 8;
            nz = (c + cper - 1) / cper;
        }
    }
    hipLaunchKernelGGL((lrn_pool_fwd_kernel<CHK, PPT, NSL, C8>), dim3(bands, (n + 7) / 8 * 8, nz), dim3(threads), lds, stream, x, p, argmax, c, h,
                       w, oh, ow, prb, (int)pplane, owp, p_halo, alpha, bias, cper, n);
    VL_LAUNCH_CHECK();
    return 0;
}

extern "C" int vl_lrn_pool_fwd(const float* x, float* p, uint8_t* argmax, int n, int c, int h, int w, int p_halo, int radius,
                               float alpha, float beta, float bias, vl_stream_t stream) {
    VL_CHECK(x && p && argmax && n > 0 && c > 0 && h >= 3 && w >= 3 && p_halo >= 0, "vl_lrn_pool_fwd: bad argument");
    VL_CHECK(radius == 2 && beta == 0.75f, "vl_lrn_pool_fwd: only depth_radius 2, beta 0.75 are built (alexnet.py:81-84)");
    VL_CHECK(n <= 65528, "vl_lrn_pool_fwd: batch %d exceeds the grid limit", n);
    const int oh = (h - 3) / 2 + 1, ow = (w - 3) / 2 + 1;
    const int owp = ow + 2 * p_halo;
    const int64_t pplane = (int64_t)(oh + 2 * p_halo) * owp;
    VL_CHECK((int64_t)(c + 16) * h * w * 4 < (1ll << 31) && (int64_t)c * pplane * 4 < (1ll << 31) && pplane < (1 << 24),
             "vl_lrn_pool_fwd: image too large for 32-bit buffer offsets");
    // Chunk of 2 channels, 2 pixels and 1 pooled output per thread: 46 registers, 13 KB of LDS -> the CU holds 4-5 workgroups of 448
    // threads.  The round-1 shape <8, 3, 6> (8-channel chunks, 214 registers, 55 KB) left ONE 320-thread workgroup = 5 waves on a CU and
    // ran LRN's ~13 VALU per element at that occupancy: layer 1 0.63 -> 0.45 ms, layer 2 0.33 -> 0.28 ms (sweep of 14 shapes on MI355X,
    // tools/pw_probe.py lrn_pool_fwd; VL_LRN_POOL_R1=1 runs the old shape for comparison).
    static const bool r1 = vl_exp_env("VL_LRN_POOL_R1") != nullptr;
    hipStream_t s = (hipStream_t)stream;
    if (r1) return launch_lrn_pool_fwd<8, 3, 6>(x, p, argmax, n, c, h, w, p_halo, alpha, bias, s);
    return launch_lrn_pool_fwd<2, 2, 1>(x, p, argmax, n, c, h, w, p_halo, alpha, bias, s);
}

/* vl_lrn_pool_fwd with the pooled output written as packed bf16 (pb: "c8" layout of the bf16 conv path, p_halo; nearest even) instead of
 * fp32 p -- the next conv's operand; argmax keeps the fp32 form's NCHW layout with p_halo. */
extern "C" int vl_lrn_pool_fwd_c8(const void* x, int x_packed, void* pb, uint8_t* argmax, int n, int c, int h, int w, int p_halo, int radius,
                                  float alpha, float beta, float bias, vl_stream_t stream) {
    VL_CHECK(x && pb && argmax && n > 0 && c > 0 && h >= 3 && w >= 3 && p_halo >= 0, "vl_lrn_pool_fwd_c8: bad argument");
    VL_CHECK(radius == 2 && beta == 0.75f, "vl_lrn_pool_fwd_c8: only depth_radius 2, beta 0.75 are built (alexnet.py:81-84)");
    VL_CHECK(n <= 65528, "vl_lrn_pool_fwd_c8: batch %d exceeds the grid limit", n);
    const int oh = (h - 3) / 2 + 1, ow = (w - 3) / 2 + 1;
    const int64_t pplane = (int64_t)(oh + 2 * p_halo) * (ow + 2 * p_halo);
    VL_CHECK((int64_t)(c + 16) * h * w * 4 < (1ll << 31) && (int64_t)((c + 7) / 8) * pplane * 16 < (1ll << 31) && pplane < (1 << 24),
             "vl_lrn_pool_fwd_c8: image too large for 32-bit buffer offsets");
    if (x_packed) return launch_lrn_pool_fwd<2, 2, 1, 2>((const float*)x, (float*)pb, argmax, n, c, h, w, p_halo, alpha, bias, (hipStream_t)stream);
    return launch_lrn_pool_fwd<2, 2, 1, 1>((const float*)x, (float*)pb, argmax, n, c, h, w, p_halo, alpha, bias, (hipStream_t)stream);
}

// ---- max-pool VALID (alexnet.py:91-98) --------------------------------------------------------
// Index decode uses 32-bit magic-number division (total element counts are < 2^31, checked on the host);
// K, S > 0 are compile-time for the 3x3/2 case the reference uses, 0 = runtime k, s.
template <int K, int S>
__global__ void maxpool_fwd_kernel(const float* __restrict__ x, float* __restrict__ y, uint8_t* __restrict__ arg, uint32_t total,
                                   int C, int H, int W, int OH, int OW, int k_, int s_, FastDiv dOHW, FastDiv dOW, FastDiv dC,
                                   int64_t ysn, int64_t ysc, int64_t ysh, int64_t ysw) {
    const int k = K ? K : k_, s = S ? S : s_;
    const int OHW = OH * OW;
    for (uint32_t e = blockIdx.x * blockDim.x + threadIdx.x; e < total; e += gridDim.x * blockDim.x) {
        const uint32_t plane = fd_div(e, dOHW);
        const uint32_t p = e - plane * OHW;
        const uint32_t oh = fd_div(p, dOW), ow = p - oh * OW;
        const uint32_t img = fd_div(plane, dC), c = plane - img * C;
        const float* xp = x + ((int64_t)plane * H + oh * s) * W + ow * s;
        float best = -INFINITY;
        int bi = 0;
#pragma unroll
        for (int i = 0; i < (K ? K : 1); ++i)
#pragma unroll
            for (int j = 0; j < (K ? K : 1); ++j) {
                if (K) {
                    const float v = xp[i * W + j];
                    if (v > best) {  // strict: the first maximum in scan order wins
                        best = v;
                        bi = i * K + j;
                    }
                }
            }
        if (!K) {
            for (int i = 0; i < k; ++i)
                for (int j = 0; j < k; ++j) {
                    const float v = xp[i * W + j];
                    if (v > best) {
                        best = v;
                        bi = i * k + j;
                    }
                }
        }
        const int64_t o = img * ysn + c * ysc + oh * ysh + ow * ysw;
        y[o] = best;
        if (arg) arg[o] = (uint8_t)bi;
    }
}

template <int K, int S>
__global__ void maxpool_bwd_kernel(const float* __restrict__ dy, const uint8_t* __restrict__ arg, float* __restrict__ dx,
                                   const float* __restrict__ mask, uint32_t total, int C, int H, int W, int OH, int OW, int k_,
                                   int s_, FastDiv dHW, FastDiv dW, FastDiv dC, int64_t ysn, int64_t ysc, int64_t ysh, int64_t ysw,
                                   int halo) {
    const int k = K ? K : k_, s = S ? S : s_;
    const int HW = H * W;
    const int wp = W + 2 * halo;
    const int64_t pp = (int64_t)(H + 2 * halo) * wp;
    for (uint32_t e = blockIdx.x * blockDim.x + threadIdx.x; e < total; e += gridDim.x * blockDim.x) {
        const uint32_t plane = fd_div(e, dHW);
        const uint32_t p = e - plane * HW;
        const int ih = (int)fd_div(p, dW), iw = (int)(p - ih * W);
        const uint32_t img = fd_div(plane, dC), c = plane - img * C;
        float acc = 0.f;
        if (!mask || mask[e] > 0.f) {
            int oh_lo = (ih - k + s) / s;  // ceil((ih - k + 1) / s) for ih-k+1 >= 0
            if (ih - k + 1 < 0) oh_lo = 0;
            int ow_lo = (iw - k + s) / s;
            if (iw - k + 1 < 0) ow_lo = 0;
            const int oh_hi = min(ih / s, OH - 1), ow_hi = min(iw / s, OW - 1);
            const int64_t base = img * ysn + c * ysc;
            for (int oh = oh_lo; oh <= oh_hi; ++oh)
                for (int ow = ow_lo; ow <= ow_hi; ++ow) {
                    const int64_t o = base + oh * ysh + ow * ysw;
                    if ((int)arg[o] == (ih - oh * s) * k + (iw - ow * s)) acc += dy[o];
                }
        }
        dx[(int64_t)plane * pp + (int64_t)(ih + halo) * wp + iw + halo] = acc;
    }
}

extern "C" int vl_maxpool_fwd(const float* x, float* y, uint8_t* argmax, int n, int c, int h, int w, int k, int s, int64_t ys_n,
                              int64_t ys_c, int64_t ys_h, int64_t ys_w, vl_stream_t stream) {
    VL_CHECK(x && y && n > 0 && c > 0 && k > 0 && s > 0 && h >= k && w >= k && k * k <= 255, "vl_maxpool_fwd: bad argument");
    const int oh = (h - k) / s + 1, ow = (w - k) / s + 1;
    const int64_t total = (int64_t)n * c * oh * ow;
    VL_CHECK(total < (1ll << 31) && (int64_t)n * c * h * w < (1ll << 40), "vl_maxpool_fwd: tensor too large");
    const dim3 grid(grid_for(total, 256, 16384));
    const FastDiv d1 = make_fastdiv(oh * ow), d2 = make_fastdiv(ow), d3 = make_fastdiv(c);
    if (k == 3 && s == 2)
        hipLaunchKernelGGL((maxpool_fwd_kernel<3, 2>), grid, dim3(256), 0, (hipStream_t)stream, x, y, argmax, (uint32_t)total, c, h, w, oh,
                           ow, k, s, d1, d2, d3, ys_n, ys_c, ys_h, ys_w);
    else
        hipLaunchKernelGGL((maxpool_fwd_kernel<0, 0>), grid, dim3(256), 0, (hipStream_t)stream, x, y, argmax, (uint32_t)total, c, h, w, oh,
                           ow, k, s, d1, d2, d3, ys_n, ys_c, ys_h, ys_w);
    VL_LAUNCH_CHECK();
    return 0;
}

// pool5's backward (3x3 / 2, pooled tensor stored (h, w, c)-flat for fc6, input gradient NCHW): in the generic kernel above a
// wave walks input columns, so its <= 4 pooled neighbours are c * 4 bytes apart -- every byte / float of the pooled tensors is
// its own cache line.  Here a workgroup stages the pooled gradient and arg-max of CB channels of one image through LDS
// (coalesced along c, which is contiguous in the source), then writes the NCHW planes coalesced along the pixels.
// Round 3: lane = pixel, channels in the loop (was: one flat element index per thread with two divisions per element): 0.355 ->
// 0.176 ms at 1024 frames (tools/pool5_probe.py; VL_MAXPOOL_GENERIC=1 runs the element-per-thread kernel).  The same treatment
// of the FORWARD (64 planes copied to LDS, lane = channel) was slower than the element-per-thread kernel (0.105 vs 0.071 ms) and
// was dropped: its strided writes are absorbed by the L2, the serial copy phase is not.
template <int CB, bool MASK>
__global__ __launch_bounds__(256) void maxpool_bwd_hwc_k3s2_kernel(const float* __restrict__ dy, const uint8_t* __restrict__ arg,
                                                                   float* __restrict__ dx, const float* __restrict__ mask, int C, int H,
                                                                   int W, int OH, int OW, int halo) {
    extern __shared__ __attribute__((aligned(16))) unsigned char pl_smem[];
    const int OHW = OH * OW, HW = H * W, SP = OHW + 1;
    uint2* sp = reinterpret_cast<uint2*>(pl_smem);                     // [CB][OHW + 1] entries {dy bits, arg-max}
    const int img = blockIdx.y, c0 = blockIdx.x * CB;
    const int nch = min(CB, C - c0);
    const float* dyp = dy + (int64_t)img * OHW * C;
    const uint8_t* ap = arg + (int64_t)img * OHW * C;
    // Round 4: every loop of this kernel was ONE load, its wait, its use -- hipcc had turned the conditional loads into branches
    // (exec-mask tests around each), 9 + 64 dependent round trips per thread.  Now: clamped addresses instead of conditions, the
    // loads of four entries / four channels issued before the first is used, selects instead of branches.
    constexpr int EU = 4;
    for (int e0 = threadIdx.x; e0 < CB * OHW; e0 += 256 * EU) {
        uint32_t dv[EU], av[EU];
#pragma unroll
        for (int u = 0; u < EU; ++u) {
            const int e = min(e0 + 256 * u, CB * OHW - 1);
            const int p = e / CB, cl = min(e - p * CB, nch - 1);       // lanes walk c: contiguous in the (h, w, c) source
            dv[u] = __float_as_uint(dyp[(int64_t)p * C + c0 + cl]);
            av[u] = (uint32_t)ap[(int64_t)p * C + c0 + cl];
        }
#pragma unroll
        for (int u = 0; u < EU; ++u) {
            const int e = e0 + 256 * u;
            const int p = e / CB, cl = e - p * CB;
            if (e < CB * OHW) sp[cl * SP + p] = cl < nch ? make_uint2(dv[u], av[u]) : make_uint2(0u, 255u);
        }
    }
    if ((int)threadIdx.x < CB) sp[threadIdx.x * SP + OHW] = make_uint2(0u, 255u);   // the pad entry unreachable windows read
    __syncthreads();
    // lane = input pixel (64 at a time), wave w takes channels w, w + 4, ...: a pixel's <= 4 windows (rows ih>>1 and one above,
    // columns iw>>1 and one to the left) are decoded ONCE per pixel chunk, the channel loop is 4 LDS reads, 4 compare-selects, the
    // mask load and the store -- no division per element
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int wp = W + 2 * halo;
    const int64_t pp = (int64_t)(H + 2 * halo) * wp;
    // (round 4) the lanes enumerate whole rows of dx's halo layout, halo columns included (they store the 0.0 a halo holds): 13-float
    // rows at a 15-float pitch left every sector partially written -- pool_lrn_bwd gained 22 % from the same change
    const int HWq = H * wp;
    for (int pc = 0; pc * 64 < HWq; ++pc) {
        const int pq = pc * 64 + lane;
        const bool inplane = pq < HWq;
        const int pcl = inplane ? pq : HWq - 1;
        const int ih = pcl / wp, iwq = pcl - ih * wp, iwr = iwq - halo;
        const bool valid = inplane && iwr >= 0 && iwr < W;
        const int iw = min(max(iwr, 0), W - 1);
        const int p = ih * W + iw;                                     // (clamped: always a pixel of the plane)
        int off[4], wl[4];
#pragma unroll
        for (int a = 0; a < 2; ++a) {
            const int oh = (ih >> 1) - a, lr = (ih & 1) + 2 * a;
#pragma unroll
            for (int b = 0; b < 2; ++b) {
                const int ow = (iw >> 1) - b, lc = (iw & 1) + 2 * b;
                const bool ok = valid && oh >= 0 && oh < OH && lr <= 2 && ow >= 0 && ow < OW && lc <= 2;
                off[a * 2 + b] = ok ? oh * OW + ow : OHW;              // entry OHW of a row: the pad, never a match
                wl[a * 2 + b] = ok ? lr * 3 + lc : 254;
            }
        }
        const int64_t dxo = (int64_t)(ih + halo) * wp + iwq;
        constexpr int CU = 4;                                          // channels per pass
        for (int cb = wave; cb < nch; cb += 4 * CU) {
            float mk[CU];
            uint2 en[CU][4];
#pragma unroll
            for (int u = 0; u < CU; ++u) {
                const int cl = min(cb + 4 * u, nch - 1);               // (clamped: a repeated channel is computed and not stored)
                if constexpr (MASK) mk[u] = mask[((int64_t)img * C + c0 + cl) * HW + p];
                else mk[u] = 1.f;
                const uint2* row = sp + cl * SP;
#pragma unroll
                for (int k = 0; k < 4; ++k) en[u][k] = row[off[k]];
            }
#pragma unroll
            for (int u = 0; u < CU; ++u) {
                const int cl = cb + 4 * u;
                float acc = 0.f;
#pragma unroll
                for (int k = 0; k < 4; ++k) acc += ((int)en[u][k].y == wl[k]) ? __uint_as_float(en[u][k].x) : 0.f;
                if (!(mk[u] > 0.f)) acc = 0.f;
                if (inplane && cl < nch) dx[((int64_t)img * C + c0 + cl) * pp + dxo] = acc;   // halo columns: no window matched, acc = 0
            }
        }
    }
}

extern "C" int vl_maxpool_bwd(const float* dy, const uint8_t* argmax, float* dx, const float* relu_mask, int n, int c, int h,
                              int w, int k, int s, int64_t ys_n, int64_t ys_c, int64_t ys_h, int64_t ys_w, int dx_halo,
                              vl_stream_t stream) {
    VL_CHECK(dy && argmax && dx && n > 0 && c > 0 && k > 0 && s > 0 && h >= k && w >= k && dx_halo >= 0, "vl_maxpool_bwd: bad argument");
    const int oh = (h - k) / s + 1, ow = (w - k) / s + 1;
    const int64_t total = (int64_t)n * c * h * w;
    VL_CHECK(total < (1ll << 31), "vl_maxpool_bwd: tensor too large");
    if (k == 3 && s == 2 && ys_c == 1 && ys_w == c && ys_h == (int64_t)ow * c && ys_n == (int64_t)oh * ow * c && n <= 65535 &&
        (size_t)64 * (oh * ow + 1) * 8 <= 48 * 1024 && !kMaxpoolGeneric) {
        // the (h, w, c)-flat pooled layout (pool5 -> fc6): LDS-transposed form
        // 64 channels per workgroup; 16 when that grid is under four workgroups per CU (128 frames: 512 workgroups of 48 serial
        // iterations per wave took 45 us where 1/8 of the 1024-frame time is 18; round 4)
        if ((int64_t)ceil_div(c, 64) * n >= 4ll * vl_device_cus()) {
            constexpr int CB = 64;
            auto k = relu_mask ? maxpool_bwd_hwc_k3s2_kernel<CB, true> : maxpool_bwd_hwc_k3s2_kernel<CB, false>;
            hipLaunchKernelGGL(k, dim3(ceil_div(c, CB), n), dim3(256), (size_t)CB * (oh * ow + 1) * 8, (hipStream_t)stream,
                               dy, argmax, dx, relu_mask, c, h, w, oh, ow, dx_halo);
        } else {
            constexpr int CB = 16;
            auto k = relu_mask ? maxpool_bwd_hwc_k3s2_kernel<CB, true> : maxpool_bwd_hwc_k3s2_kernel<CB, false>;
            hipLaunchKernelGGL(k, dim3(ceil_div(c, CB), n), dim3(256), (size_t)CB * (oh * ow + 1) * 8, (hipStream_t)stream,
                               dy, argmax, dx, relu_mask, c, h, w, oh, ow, dx_halo);
        }
        VL_LAUNCH_CHECK();
        return 0;
    }
    const dim3 grid(grid_for(total, 256, 16384));
    const FastDiv d1 = make_fastdiv(h * w), d2 = make_fastdiv(w), d3 = make_fastdiv(c);
    if (k == 3 && s == 2)
        hipLaunchKernelGGL((maxpool_bwd_kernel<3, 2>), grid, dim3(256), 0, (hipStream_t)stream, dy, argmax, dx, relu_mask, (uint32_t)total,
                           c, h, w, oh, ow, k, s, d1, d2, d3, ys_n, ys_c, ys_h, ys_w, dx_halo);
    else
        hipLaunchKernelGGL((maxpool_bwd_kernel<0, 0>), grid, dim3(256), 0, (hipStream_t)stream, dy, argmax, dx, relu_mask, (uint32_t)total,
                           c, h, w, oh, ow, k, s, d1, d2, d3, ys_n, ys_c, ys_h, ys_w, dx_halo);
    VL_LAUNCH_CHECK();
    return 0;
}

// ---- bias gradients ---------------------------------------------------------------------------
__device__ __forceinline__ float block_sum_256(float v, float* sm) {
    v = wave_sum(v);
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    if (lane == 0) sm[wv] = v;
    __syncthreads();
    const float r = sm[0] + sm[1] + sm[2] + sm[3];
    __syncthreads();
    return r;
}

// grid (C, S): block (c, s) sums channel c over images [s*per, (s+1)*per) -> ws[s*C + c]
__global__ void bias_grad_stage1(const float* __restrict__ dy, float* __restrict__ ws, int n, int C, int HW, int per) {
    __shared__ float sm[4];
    const int c = blockIdx.x, s = blockIdx.y;
    const int n0 = s * per, n1 = min(n, n0 + per);
    float acc = 0.f;
    // eight images' loads in flight per pass (one image per pass was one dependent round trip per image: conv3's 15 x 15 planes, 36
    // images per workgroup, ran at 3 TB/s -- latency, not bandwidth; round 4)
    const int64_t istride = (int64_t)C * HW;
    for (int img = n0; img < n1; img += 8) {
        const float* p = dy + ((int64_t)img * C + c) * HW;
        const int cnt = min(8, n1 - img);
        for (int i = threadIdx.x; i < HW; i += 256) {
            float v[8];
#pragma unroll
            for (int e = 0; e < 8; ++e) v[e] = e < cnt ? p[e * istride + i] : 0.f;
#pragma unroll
            for (int e = 0; e < 8; ++e) acc += v[e];
        }
    }
    acc = block_sum_256(acc, sm);
    if (threadIdx.x == 0) ws[s * C + c] = acc;
}

__global__ void sum_partials_kernel(const float* __restrict__ ws, float* __restrict__ out, int count, int S) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= count) return;
    float a = 0.f;
    int s = 0;
    for (; s + 8 <= S; s += 8) {                                       // eight loads in flight, added in slice order
        float v[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) v[e] = ws[(int64_t)(s + e) * count + c];
#pragma unroll
        for (int e = 0; e < 8; ++e) a += v[e];
    }
    for (; s < S; ++s) a += ws[(int64_t)s * count + c];
    out[c] = a;
}

extern "C" int vl_bias_grad_nchw(const float* dy, float* db, float* ws, int n, int c, int hw, vl_stream_t stream) {
    VL_CHECK(dy && db && ws && n > 0 && c > 0 && hw > 0, "vl_bias_grad_nchw: bad argument");
    // slices of >= 8192 elements per channel, so that the second stage adds a handful of partials (S = 64 for any n cost 15 us there)
    const int64_t want = ((int64_t)n * hw + 8191) / 8192;
    const int S = want < 1 ? 1 : want > 64 ? 64 : want > n ? n : (int)want;
    const int per = ceil_div(n, S);
    const int S2 = ceil_div(n, per);
    hipLaunchKernelGGL(bias_grad_stage1, dim3(c, S2), dim3(256), 0, (hipStream_t)stream, dy, S2 == 1 ? db : ws, n, c, hw, per);
    VL_LAUNCH_CHECK();
    if (S2 > 1) {
        hipLaunchKernelGGL(sum_partials_kernel, dim3(ceil_div(c, 256)), dim3(256), 0, (hipStream_t)stream, ws, db, c, S2);
        VL_LAUNCH_CHECK();
    }
    return 0;
}

// grid (ceil(ncol / 32), S): a workgroup sums 32 columns over rows [s*per, (s+1)*per) -- 8 row groups of 32 lanes (whole 128-byte
// lines), combined through LDS in a fixed order -> dst[s*ncol + j].  With S = 1 dst is the result itself (one launch: the
// classifier / LSTM / fc6 bias gradients of a 128-frame shard were two launches of 6 + 17 us each).
__global__ __launch_bounds__(256) void colsum_stage1(const float* __restrict__ a, int64_t lda, float* __restrict__ dst, int m, int ncol, int per) {
    __shared__ float part[8][32];
    const int lx = threadIdx.x & 31, g = threadIdx.x >> 5;
    const int j = blockIdx.x * 32 + lx;
    const int s = blockIdx.y;
    const int r1 = min(m, (s + 1) * per);
    float acc = 0.f;
    if (j < ncol) {
        int r = s * per + g;
        for (; r + 24 < r1; r += 32) {
            const float v0 = a[(int64_t)r * lda + j], v1 = a[(int64_t)(r + 8) * lda + j], v2 = a[(int64_t)(r + 16) * lda + j],
                        v3 = a[(int64_t)(r + 24) * lda + j];
            acc += v0; acc += v1; acc += v2; acc += v3;
        }
        for (; r < r1; r += 8) acc += a[(int64_t)r * lda + j];
    }
    part[g][lx] = acc;
    __syncthreads();
    if (g == 0 && j < ncol) {
        float t = 0.f;
#pragma unroll
        for (int i = 0; i < 8; ++i) t += part[i][lx];
        dst[(int64_t)s * ncol + j] = t;
    }
}

extern "C" int vl_colsum(const float* a, int64_t lda, float* out, float* ws, int m, int n, vl_stream_t stream) {
    VL_CHECK(a && out && ws && m > 0 && n > 0 && lda >= n, "vl_colsum: bad argument");
    const int S = ceil_div(m, 256) < 64 ? ceil_div(m, 256) : 64;
    const int per = ceil_div(m, S);
    const int S2 = ceil_div(m, per);
    hipLaunchKernelGGL(colsum_stage1, dim3(ceil_div(n, 32), S2), dim3(256), 0, (hipStream_t)stream, a, lda, S2 == 1 ? out : ws, m, n, per);
    VL_LAUNCH_CHECK();
    if (S2 > 1) {
        hipLaunchKernelGGL(sum_partials_kernel, dim3(ceil_div(n, 256)), dim3(256), 0, (hipStream_t)stream, ws, out, n, S2);
        VL_LAUNCH_CHECK();
    }
    return 0;
}

// ---- LSTM gate pointwise (TF BasicLSTMCell; lstm.py:17) ---------------------------------------
__device__ __forceinline__ float sigmoidf_(float x) { return 1.f / (1.f + expf(-x)); }

__global__ void lstm_step_fwd_kernel(const float* __restrict__ gx, const float* __restrict__ gh, float* __restrict__ act,
                                     float* __restrict__ cseq, float* __restrict__ hseq, float* __restrict__ hprev, int batch,
                                     int T, int t, int H, float forget_bias) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= batch * H) return;
    const int b = e / H, u = e - b * H;
    const int64_t r = (int64_t)b * T + t;
    const float* zx = gx + r * 4 * H;
    float zi = zx[u], zj = zx[H + u], zf = zx[2 * H + u], zo = zx[3 * H + u];
    if (gh) {
        const float* zh = gh + (int64_t)b * 4 * H;
        zi += zh[u];
        zj += zh[H + u];
        zf += zh[2 * H + u];
        zo += zh[3 * H + u];
    }
    const float gi = sigmoidf_(zi), gj = tanhf(zj), gf = sigmoidf_(zf + forget_bias), go = sigmoidf_(zo);
    const float cp = t > 0 ? cseq[(r - 1) * H + u] : 0.f;
    const float hp = t > 0 ? hseq[(r - 1) * H + u] : 0.f;
    const float c = cp * gf + gi * gj;
    const float h = tanhf(c) * go;
    float* a = act + r * 4 * H;
    a[u] = gi;
    a[H + u] = gj;
    a[2 * H + u] = gf;
    a[3 * H + u] = go;
    cseq[r * H + u] = c;
    hseq[r * H + u] = h;
    hprev[r * H + u] = hp;
}

__global__ void lstm_step_bwd_kernel(const float* __restrict__ dout, const float* __restrict__ dh_next,
                                     const float* __restrict__ act, const float* __restrict__ cseq, float* __restrict__ dc,
                                     float* __restrict__ dz, int batch, int T, int t, int H) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= batch * H) return;
    const int b = e / H, u = e - b * H;
    const int64_t r = (int64_t)b * T + t;
    float dh = dout ? dout[r * H + u] : 0.f;
    if (dh_next) dh += dh_next[(int64_t)b * H + u];
    const float* a = act + r * 4 * H;
    const float gi = a[u], gj = a[H + u], gf = a[2 * H + u], go = a[3 * H + u];
    const float c = cseq[r * H + u];
    const float cp = t > 0 ? cseq[(r - 1) * H + u] : 0.f;
    const float tc = tanhf(c);
    const float d_o = dh * tc;
    const float dcv = dc[e] + dh * go * (1.f - tc * tc);
    float* z = dz + r * 4 * H;
    z[u] = dcv * gj * gi * (1.f - gi);
    z[H + u] = dcv * gi * (1.f - gj * gj);
    z[2 * H + u] = dcv * cp * gf * (1.f - gf);
    z[3 * H + u] = d_o * go * (1.f - go);
    dc[e] = dcv * gf;
}

extern "C" int vl_lstm_step_fwd(const float* gx, const float* gh, float* act, float* cseq, float* hseq, float* hprev, int batch,
                                int T, int t, int H, float forget_bias, vl_stream_t stream) {
    VL_CHECK(gx && act && cseq && hseq && hprev, "vl_lstm_step_fwd: null argument");
    VL_CHECK(batch > 0 && H > 0 && T > 0 && t >= 0 && t < T, "vl_lstm_step_fwd: bad shape");
    VL_CHECK(gh || t == 0, "vl_lstm_step_fwd: gh required for t > 0");
    hipLaunchKernelGGL(lstm_step_fwd_kernel, dim3(ceil_div((int64_t)batch * H, 256)), dim3(256), 0, (hipStream_t)stream, gx, gh,
                       act, cseq, hseq, hprev, batch, T, t, H, forget_bias);
    VL_LAUNCH_CHECK();
    return 0;
}

extern "C" int vl_lstm_step_bwd(const float* dout, const float* dh_next, const float* act, const float* cseq, float* dc,
                                float* dz, int batch, int T, int t, int H, vl_stream_t stream) {
    VL_CHECK(act && cseq && dc && dz, "vl_lstm_step_bwd: null argument");
    VL_CHECK(batch > 0 && H > 0 && T > 0 && t >= 0 && t < T, "vl_lstm_step_bwd: bad shape");
    hipLaunchKernelGGL(lstm_step_bwd_kernel, dim3(ceil_div((int64_t)batch * H, 256)), dim3(256), 0, (hipStream_t)stream, dout,
                       dh_next, act, cseq, dc, dz, batch, T, t, H);
    VL_LAUNCH_CHECK();
    return 0;
}

// ---- persistent per-clip LSTM recurrence ------------------------------------------------------------
// Clips are independent, so the whole T-step recurrence of a clip runs inside ONE workgroup with no
// inter-workgroup traffic: lane u owns hidden unit u (all four gates), h_{t-1} / dz_t are exchanged through
// LDS, and the recurrent weights (kh = kernel[D:], [H][4H]) are streamed from L2 every step (1 MB for H = 256).
// Loads are staged through a register array so a whole batch is in flight (hipcc otherwise waits after every
// load), and every clip starts at a different row so the CUs do not hit one L2 channel in lockstep.
// Replaces T x {vl_gemm(M = clips), vl_lstm_step_*} launches.
// seq_len (nullable, vltf.h "per-clip sequence lengths"): the workgroup IS the clip, so it runs the first L = seq_len[b] steps only and
// fills the dead rows t >= L afterwards (forward: act 0, cseq = the carried c, hseq 0, hprev = the carried h; backward: dz 0).
template <bool BWD>
__global__ void lstm_seq_kernel(const float* __restrict__ gx, const float* __restrict__ kmat, float* __restrict__ act,
                                float* __restrict__ cseq, float* __restrict__ hseq, float* __restrict__ hprev,
                                const float* __restrict__ dout, float* __restrict__ dz, int T, int H, float forget_bias, int KQ,
                                const float* __restrict__ h0, const float* __restrict__ c0, float* __restrict__ dh0,
                                float* __restrict__ dc0, const int32_t* __restrict__ seq_len) {
    // blockDim = KQ * HP threads (HP = H rounded up to the wave): thread (u, kq) accumulates the kq-th slice of the recurrent
    // reduction for hidden unit u; the KQ partial sums meet in LDS and the kq = 0 threads do the gate math.  The recurrence is a
    // chain of T dependent steps whose length is set by load latency, not bandwidth (1 MB of weights per step from L2): splitting
    // the reduction four ways cuts the dependent load batches per step from 16 to 4.
    extern __shared__ __attribute__((aligned(16))) float sm[];
    const int HP = blockDim.x / KQ;
    const int b = blockIdx.x, u = threadIdx.x % HP, kq = threadIdx.x / HP;
    const bool live = u < H;
    const int uc = live ? u : 0;                       // clamped: idle lanes load valid addresses, results unused
    const int H4 = 4 * H;
    const int L = seq_len ? min(max(seq_len[b], 0), T) : T;   // live steps of this clip
    constexpr int KB = 16;
    if (!BWD) {
        float* hs = sm;                                // [H] h_{t-1}
        float* part = sm + H;                          // [KQ][4][H] partial gate pre-activations
        float c = (c0 && live) ? c0[(int64_t)b * H + u] : 0.f;
        for (int i = threadIdx.x; i < H; i += blockDim.x) hs[i] = h0 ? h0[(int64_t)b * H + i] : 0.f;
        __syncthreads();
        const bool rec0 = h0 != nullptr;               // an initial state makes step 0 a full recurrent step
        const int klen = (H + KQ - 1) / KQ, k0 = kq * klen, k1 = min(H, k0 + klen);
        const int nb = (k1 - k0) / KB, rot = (b * 5) % (nb > 0 ? nb : 1);
        for (int t = 0; t < L; ++t) {
            const int64_t r = (int64_t)b * T + t;
            float z[4] = {0.f, 0.f, 0.f, 0.f};
            if (t > 0 || rec0) {
                for (int ib = 0; ib < nb; ++ib) {
                    const int kb = k0 + ((ib + rot) % nb) * KB;
                    float w[KB][4];
#pragma unroll
                    for (int kk = 0; kk < KB; ++kk)
#pragma unroll
                        for (int q = 0; q < 4; ++q) w[kk][q] = kmat[(int64_t)(kb + kk) * H4 + q * H + uc];
#pragma unroll
                    for (int kk = 0; kk < KB; ++kk) {
                        const float hk = hs[kb + kk];
#pragma unroll
                        for (int q = 0; q < 4; ++q) z[q] += hk * w[kk][q];
                    }
                }
                for (int k = k0 + nb * KB; k < k1; ++k) {
                    const float hk = hs[k];
#pragma unroll
                    for (int q = 0; q < 4; ++q) z[q] += hk * kmat[(int64_t)k * H4 + q * H + uc];
                }
                if (live)
#pragma unroll
                    for (int q = 0; q < 4; ++q) part[(kq * 4 + q) * H + u] = z[q];
            }
            const float hp = hs[uc];
            __syncthreads();                           // partial sums complete; everyone has consumed h_{t-1}
            if (live && kq == 0) {
                float zz[4];
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    zz[q] = gx[r * H4 + q * H + u];
                    if (t > 0 || rec0)
                        for (int j = 0; j < KQ; ++j) zz[q] += part[(j * 4 + q) * H + u];    // fixed order: reproducible
                }
                const float gi = sigmoidf_(zz[0]), gj = tanhf(zz[1]), gf = sigmoidf_(zz[2] + forget_bias), go = sigmoidf_(zz[3]);
                c = c * gf + gi * gj;
                const float h = tanhf(c) * go;
                hs[u] = h;
                float* a = act + r * H4 + u;
                a[0] = gi; a[H] = gj; a[2 * H] = gf; a[3 * H] = go;
                cseq[r * H + u] = c;
                hseq[r * H + u] = h;
                hprev[r * H + u] = hp;
            }
            __syncthreads();                           // h_t visible before the next step
        }
        if (live && kq == 0) {                         // dead rows: state carried, output zero (hs[u] is this thread's own last write)
            const float hc = hs[u];
            for (int t = L; t < T; ++t) {
                const int64_t r = (int64_t)b * T + t;
                float* a = act + r * H4 + u;
                a[0] = 0.f; a[H] = 0.f; a[2 * H] = 0.f; a[3 * H] = 0.f;
                cseq[r * H + u] = c;
                hseq[r * H + u] = 0.f;
                hprev[r * H + u] = hc;
            }
        }
    } else {
        // kmat = khT [4H][H]: dh_prev[u] = sum_g dz[g] * khT[g][u]
        float* zs = sm;                                // [4H] dz_t
        float* part = sm + H4;                         // [KQ][H] partial dh
        float dc = 0.f, dh = 0.f;
        const int glen = (H4 + KQ - 1) / KQ, g0 = kq * glen, g1 = min(H4, g0 + glen);
        const int nb = (g1 - g0) / KB, rot = (b * 5) % (nb > 0 ? nb : 1);
        if (live && kq == 0)                           // dead rows: dz = 0, nothing read
            for (int t = L; t < T; ++t) {
                float* zp = dz + ((int64_t)b * T + t) * H4 + u;
                zp[0] = 0.f; zp[H] = 0.f; zp[2 * H] = 0.f; zp[3 * H] = 0.f;
            }
        for (int t = L - 1; t >= 0; --t) {
            const int64_t r = (int64_t)b * T + t;
            if (live && kq == 0) {
                const float din = (dout ? dout[r * H + u] : 0.f) + dh;
                const float* a = act + r * H4 + u;
                const float gi = a[0], gj = a[H], gf = a[2 * H], go = a[3 * H];
                const float cc = cseq[r * H + u];
                const float cp = t > 0 ? cseq[(r - 1) * H + u] : (c0 ? c0[(int64_t)b * H + u] : 0.f);
                const float tc = tanhf(cc);
                const float d_o = din * tc;
                const float dcv = dc + din * go * (1.f - tc * tc);
                const float zi = dcv * gj * gi * (1.f - gi), zj = dcv * gi * (1.f - gj * gj);
                const float zf = dcv * cp * gf * (1.f - gf), zo = d_o * go * (1.f - go);
                dc = dcv * gf;
                float* zp = dz + r * H4 + u;
                zp[0] = zi; zp[H] = zj; zp[2 * H] = zf; zp[3 * H] = zo;
                zs[u] = zi; zs[H + u] = zj; zs[2 * H + u] = zf; zs[3 * H + u] = zo;
            }
            __syncthreads();                           // dz_t complete in LDS
            if (t > 0 || dh0) {
                float acc = 0.f;
                for (int ib = 0; ib < nb; ++ib) {
                    const int g = g0 + ((ib + rot) % nb) * KB;
                    float w[KB];
#pragma unroll
                    for (int gg = 0; gg < KB; ++gg) w[gg] = kmat[(int64_t)(g + gg) * H + uc];
#pragma unroll
                    for (int gg = 0; gg < KB; ++gg) acc += zs[g + gg] * w[gg];
                }
                for (int g = g0 + nb * KB; g < g1; ++g) acc += zs[g] * kmat[(int64_t)g * H + uc];
                if (live) part[kq * H + u] = acc;
            }
            __syncthreads();                           // partial dh complete; dz_t consumed before it is overwritten
            if ((t > 0 || dh0) && live && kq == 0) {
                float acc = 0.f;
                for (int j = 0; j < KQ; ++j) acc += part[j * H + u];
                dh = acc;
            }
            // (the next iteration's first barrier separates these reads of `part` from its next writes)
        }
        if (live && kq == 0) {
            if (dh0) dh0[(int64_t)b * H + u] = dh;
            if (dc0) dc0[(int64_t)b * H + u] = dc;
        }
    }
}

// threads per workgroup: H rounded up to the wave, times the reduction split (4 when that fits a 1024-thread workgroup)
static int lstm_seq_hp(int H) { return ((H + 63) / 64) * 64; }
static int lstm_seq_kq(int H) { return lstm_seq_hp(H) * 4 <= 1024 ? 4 : (lstm_seq_hp(H) * 2 <= 1024 ? 2 : 1); }


// Per-clip form: the fallback of vl_lstm_seq_fwd / _bwd (lstm_cluster.hip) for hidden sizes its LDS-resident weight slices do
// not hold (H > 512), and the A/B reference of the cluster form (VL_LSTM_PERCLIP=1).
int vl_lstm_perclip_fwd(const float* gx, const float* kh, const float* h0, const float* c0, float* act, float* cseq, float* hseq,
                        float* hprev, int batch, int T, int H, float forget_bias, const int32_t* seq_len, hipStream_t stream) {
    const int kq = lstm_seq_kq(H);
    hipLaunchKernelGGL((lstm_seq_kernel<false>), dim3(batch), dim3(lstm_seq_hp(H) * kq), (size_t)(1 + 4 * kq) * H * sizeof(float),
                       stream, gx, kh, act, cseq, hseq, hprev, (const float*)nullptr, (float*)nullptr, T, H, forget_bias, kq, h0, c0,
                       (float*)nullptr, (float*)nullptr, seq_len);
    VL_LAUNCH_CHECK();
    return 0;
}

int vl_lstm_perclip_bwd(const float* dout, const float* kh_t, const float* act, const float* cseq, const float* c0, float* dz,
                        float* dh0, float* dc0, int batch, int T, int H, const int32_t* seq_len, hipStream_t stream) {
    const int kq = lstm_seq_kq(H);
    hipLaunchKernelGGL((lstm_seq_kernel<true>), dim3(batch), dim3(lstm_seq_hp(H) * kq), (size_t)(4 + kq) * H * sizeof(float),
                       stream, (const float*)nullptr, kh_t, const_cast<float*>(act), const_cast<float*>(cseq),
                       (float*)nullptr, (float*)nullptr, dout, dz, T, H, 0.f, kq, (const float*)nullptr, c0, dh0, dc0, seq_len);
    VL_LAUNCH_CHECK();
    return 0;
}

__global__ void transpose2d_kernel(const float* __restrict__ src, float* __restrict__ dst, int rows, int cols, int64_t ld) {
    __shared__ float tile[32][33];
    const int bx = blockIdx.x * 32, by = blockIdx.y * 32;
    for (int i = threadIdx.y; i < 32; i += blockDim.y) {
        const int r = by + i, c = bx + threadIdx.x;
        tile[i][threadIdx.x] = (r < rows && c < cols) ? src[(int64_t)r * ld + c] : 0.f;
    }
    __syncthreads();
    for (int i = threadIdx.y; i < 32; i += blockDim.y) {
        const int r = bx + i, c = by + threadIdx.x;     // dst is [cols][rows]
        if (r < cols && c < rows) dst[(int64_t)r * rows + c] = tile[threadIdx.x][i];
    }
}

extern "C" int vl_transpose(const float* src, int64_t ld, float* dst, int rows, int cols, vl_stream_t stream) {
    VL_CHECK(src && dst && rows > 0 && cols > 0 && ld >= cols, "vl_transpose: bad argument");
    hipLaunchKernelGGL(transpose2d_kernel, dim3(ceil_div(cols, 32), ceil_div(rows, 32)), dim3(32, 8), 0, (hipStream_t)stream, src,
                       dst, rows, cols, ld);
    VL_LAUNCH_CHECK();
    return 0;
}

// ---- temporal fusion (tf_util.py:4-30) --------------------------------------------------------
// seq_len (nullable): clip b fuses its first L = seq_len[b] steps only, as an L-step model would (`last` = step L - 1, `avg` = sum / L);
// the backward writes zeros to the dead rows.  nullptr: L = T.
__device__ __forceinline__ int fusion_len(const int32_t* __restrict__ seq_len, int b, int T) {
    return seq_len ? min(max(seq_len[b], 1), T) : T;
}

__global__ void temporal_fusion_fwd_kernel(const float* __restrict__ x, float* __restrict__ y, int batch, int T, int H,
                                           int method, const int32_t* __restrict__ seq_len) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= batch * H) return;
    const int b = e / H, u = e - b * H;
    const int L = fusion_len(seq_len, b, T);
    const float* p = x + (int64_t)b * T * H + u;
    if (method == 1) {
        y[e] = p[(int64_t)(L - 1) * H];
    } else {
        float a = 0.f;
        for (int t = 0; t < L; ++t) a += p[(int64_t)t * H];
        y[e] = a / (float)L;
    }
}

__global__ void temporal_fusion_bwd_kernel(const float* __restrict__ dy, float* __restrict__ dx, int batch, int T, int H,
                                           int method, const int32_t* __restrict__ seq_len) {
    const int64_t total = (int64_t)batch * T * H;
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (int64_t)gridDim.x * blockDim.x) {
        const int u = (int)(e % H);
        const int t = (int)((e / H) % T);
        const int b = (int)(e / ((int64_t)H * T));
        const float g = dy[(int64_t)b * H + u];
        const int L = fusion_len(seq_len, b, T);
        dx[e] = method == 1 ? (t == L - 1 ? g : 0.f) : (t < L ? g / (float)L : 0.f);
    }
}

static int temporal_fusion_fwd(const float* x, float* y, int batch, int T, int H, int method, const int32_t* seq_len, hipStream_t stream) {
    hipLaunchKernelGGL(temporal_fusion_fwd_kernel, dim3(ceil_div((int64_t)batch * H, 256)), dim3(256), 0, stream, x, y, batch, T, H,
                       method, seq_len);
    VL_LAUNCH_CHECK();
    return 0;
}

static int temporal_fusion_bwd(const float* dy, float* dx, int batch, int T, int H, int method, const int32_t* seq_len, hipStream_t stream) {
    hipLaunchKernelGGL(temporal_fusion_bwd_kernel, dim3(grid_for((int64_t)batch * T * H, 256, 4096)), dim3(256), 0, stream, dy, dx, batch,
                       T, H, method, seq_len);
    VL_LAUNCH_CHECK();
    return 0;
}

extern "C" int vl_temporal_fusion_fwd(const float* x, float* y, int batch, int T, int H, int method, vl_stream_t stream) {
    VL_CHECK(x && y && batch > 0 && T > 0 && H > 0 && (method == 0 || method == 1), "vl_temporal_fusion_fwd: bad argument");
    return temporal_fusion_fwd(x, y, batch, T, H, method, nullptr, (hipStream_t)stream);
}

extern "C" int vl_temporal_fusion_fwd_len(const float* x, float* y, int batch, int T, int H, int method, const int32_t* seq_len,
                                          vl_stream_t stream) {
    VL_CHECK(x && y && batch > 0 && T > 0 && H > 0 && (method == 0 || method == 1), "vl_temporal_fusion_fwd_len: bad argument");
    return temporal_fusion_fwd(x, y, batch, T, H, method, seq_len, (hipStream_t)stream);
}

extern "C" int vl_temporal_fusion_bwd(const float* dy, float* dx, int batch, int T, int H, int method, vl_stream_t stream) {
    VL_CHECK(dy && dx && batch > 0 && T > 0 && H > 0 && (method == 0 || method == 1), "vl_temporal_fusion_bwd: bad argument");
    return temporal_fusion_bwd(dy, dx, batch, T, H, method, nullptr, (hipStream_t)stream);
}

extern "C" int vl_temporal_fusion_bwd_len(const float* dy, float* dx, int batch, int T, int H, int method, const int32_t* seq_len,
                                          vl_stream_t stream) {
    VL_CHECK(dy && dx && batch > 0 && T > 0 && H > 0 && (method == 0 || method == 1), "vl_temporal_fusion_bwd_len: bad argument");
    return temporal_fusion_bwd(dy, dx, batch, T, H, method, seq_len, (hipStream_t)stream);
}

// ---- attention pooling over time (fusion `attn`; vltf.h) -----------------------------------------------------------
// One workgroup of ATTN_THREADS per clip, no atomics, every sum in one fixed order: a clip's outputs are a function of that clip's
// inputs alone.  Rows t >= L (fusion_len) of h, u and s are never read.  T <= ATTN_MAX_T: a clip's scores live in LDS.
#define ATTN_THREADS 256
#define ATTN_MAX_T 1024

// softmax pieces of e[0..L) in LDS, computed by EVERY wave on its own (same order, same bits): no exchange between waves
__device__ __forceinline__ void attn_softmax_stats(const float* e, int L, int lane, float& mx, float& sum) {
    float m = -INFINITY;
    for (int t = lane; t < L; t += 64) m = fmaxf(m, e[t]);
    mx = wave_max(m);
    float z = 0.f;
    for (int t = lane; t < L; t += 64) z += expf(e[t] - mx);
    sum = wave_sum(z);
}

__global__ __launch_bounds__(ATTN_THREADS) void attn_pool_fwd_kernel(const float* u, const float* __restrict__ c,
                                                                     const float* __restrict__ h, const int32_t* __restrict__ seq_len,
                                                                     float* s, float* __restrict__ alpha, float* __restrict__ y, int T,
                                                                     int HO, int A) {
    __shared__ float e[ATTN_MAX_T];
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int L = fusion_len(seq_len, b, T);
    const float* ub = u + (int64_t)b * T * A;              // (s may alias u: element [t][a] is read, then written, by one thread)
    float* sb = s + (int64_t)b * T * A;
    // scores: one wave per step, lanes over A in a fixed order, then the shuffle tree
    for (int t = wave; t < T; t += ATTN_THREADS / 64) {
        if (t < L) {
            float acc = 0.f;
            for (int a = lane; a < A; a += 64) {
                const float v = tanhf(ub[(int64_t)t * A + a]);
                sb[(int64_t)t * A + a] = v;
                acc = __fmaf_rn(v, c[a], acc);
            }
            acc = wave_sum(acc);
            if (lane == 0) e[t] = acc;
        } else {
            for (int a = lane; a < A; a += 64) sb[(int64_t)t * A + a] = 0.f;
        }
    }
    __syncthreads();
    float mx, z;
    attn_softmax_stats(e, L, lane, mx, z);
    __syncthreads();                                        // every wave has read the scores: they become the weights in place
    for (int t = tid; t < T; t += ATTN_THREADS) {
        const float w = t < L ? expf(e[t] - mx) / z : 0.f;
        e[t] = w;
        alpha[(int64_t)b * T + t] = w;
    }
    __syncthreads();
    const float* hb = h + (int64_t)b * T * HO;
    for (int col = tid; col < HO; col += ATTN_THREADS) {    // a thread per column, t ascending: coalesced rows of h
        float acc = 0.f;
        for (int t = 0; t < L; ++t) acc = __fmaf_rn(e[t], hb[(int64_t)t * HO + col], acc);
        y[(int64_t)b * HO + col] = acc;
    }
}

__global__ __launch_bounds__(ATTN_THREADS) void attn_pool_bwd_kernel(const float* __restrict__ dy, const float* __restrict__ h,
                                                                     const float* __restrict__ s, const float* __restrict__ alpha,
                                                                     const float* __restrict__ c, const int32_t* __restrict__ seq_len,
                                                                     float* __restrict__ du, float* __restrict__ dh,
                                                                     float* __restrict__ dcp, int T, int HO, int A) {
    __shared__ float al[ATTN_MAX_T], da[ATTN_MAX_T], de[ATTN_MAX_T];
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int L = fusion_len(seq_len, b, T);
    const float* hb = h + (int64_t)b * T * HO;
    const float* dyb = dy + (int64_t)b * HO;
    for (int t = tid; t < L; t += ATTN_THREADS) al[t] = alpha[(int64_t)b * T + t];
    // da_t = dy . h_t: one wave per live step
    for (int t = wave; t < L; t += ATTN_THREADS / 64) {
        float acc = 0.f;
        for (int col = lane; col < HO; col += 64) acc = __fmaf_rn(dyb[col], hb[(int64_t)t * HO + col], acc);
        acc = wave_sum(acc);
        if (lane == 0) da[t] = acc;
    }
    __syncthreads();
    float dot = 0.f;                                        // sum_r alpha_r da_r, by every wave on its own (same order, same bits)
    for (int t = lane; t < L; t += 64) dot = __fmaf_rn(al[t], da[t], dot);
    dot = wave_sum(dot);
    for (int t = tid; t < L; t += ATTN_THREADS) de[t] = al[t] * (da[t] - dot);
    __syncthreads();
    const float* sb = s + (int64_t)b * T * A;
    float* dub = du + (int64_t)b * T * A;
    for (int a = tid; a < A; a += ATTN_THREADS) {           // a thread per column of s / du, t ascending
        const float ca = c[a];
        float acc = 0.f;
        for (int t = 0; t < T; ++t) {
            float g = 0.f;
            if (t < L) {
                const float v = sb[(int64_t)t * A + a];
                g = de[t] * ca * (1.f - v * v);
                acc = __fmaf_rn(de[t], v, acc);
            }
            dub[(int64_t)t * A + a] = g;
        }
        dcp[(int64_t)b * A + a] = acc;
    }
    float* dhb = dh + (int64_t)b * T * HO;
    for (int col = tid; col < HO; col += ATTN_THREADS) {
        const float g = dyb[col];
        for (int t = 0; t < T; ++t) dhb[(int64_t)t * HO + col] = t < L ? al[t] * g : 0.f;
    }
}

extern "C" int vl_attn_pool_fwd(const float* u, const float* c, const float* h, const int32_t* seq_len, float* s, float* alpha, float* y,
                                int batch, int T, int HO, int A, vl_stream_t stream) {
    VL_CHECK(u && c && h && s && alpha && y, "vl_attn_pool_fwd: null pointer");
    VL_CHECK(batch > 0 && T > 0 && HO > 0 && A > 0, "vl_attn_pool_fwd: batch %d, T %d, HO %d, A %d must be positive", batch, T, HO, A);
    VL_CHECK(T <= ATTN_MAX_T, "vl_attn_pool_fwd: T %d exceeds %d (a clip's scores live in LDS)", T, ATTN_MAX_T);
    hipLaunchKernelGGL(attn_pool_fwd_kernel, dim3(batch), dim3(ATTN_THREADS), 0, (hipStream_t)stream, u, c, h, seq_len, s, alpha, y, T,
                       HO, A);
    VL_LAUNCH_CHECK();
    return 0;
}

extern "C" int vl_attn_pool_bwd(const float* dy, const float* h, const float* s, const float* alpha, const float* c,
                                const int32_t* seq_len, float* du, float* dh, float* dcp, int batch, int T, int HO, int A,
                                vl_stream_t stream) {
    VL_CHECK(dy && h && s && alpha && c && du && dh && dcp, "vl_attn_pool_bwd: null pointer");
    VL_CHECK(batch > 0 && T > 0 && HO > 0 && A > 0, "vl_attn_pool_bwd: batch %d, T %d, HO %d, A %d must be positive", batch, T, HO, A);
    VL_CHECK(T <= ATTN_MAX_T, "vl_attn_pool_bwd: T %d exceeds %d (a clip's scores live in LDS)", T, ATTN_MAX_T);
    hipLaunchKernelGGL(attn_pool_bwd_kernel, dim3(batch), dim3(ATTN_THREADS), 0, (hipStream_t)stream, dy, h, s, alpha, c, seq_len, du, dh,
                       dcp, T, HO, A);
    VL_LAUNCH_CHECK();
    return 0;
}

// ---- dropout (lstm.py:50-56; splitmix64: common.h) ---------------------------------------------
// one body for the eager kernel and the step-state one (vl_dropout_fwd_st): only where the seed comes from differs
// (the grid-stride start and step come from the kernel: blockDim read there, where the compiler knows the work-group size is uniform)
__device__ __forceinline__ void dropout_fwd_body(const float* __restrict__ x, float* __restrict__ y, uint8_t* __restrict__ mask, int64_t count,
                                                 float keep, uint64_t seed, int64_t e0, int64_t step) {
    for (int64_t e = e0; e < count; e += step) {
        const uint64_t h = splitmix64(seed ^ splitmix64((uint64_t)e));
        const float uni = (float)(h >> 40) * (1.0f / 16777216.0f);
        const uint8_t m = uni < keep ? 1 : 0;
        mask[e] = m;
        y[e] = m ? x[e] / keep : 0.f;
    }
}

__global__ void dropout_fwd_kernel(const float* __restrict__ x, float* __restrict__ y, uint8_t* __restrict__ mask, int64_t count,
                                   float keep, uint64_t seed) {
    dropout_fwd_body(x, y, mask, count, keep, seed, (int64_t)blockIdx.x * blockDim.x + threadIdx.x, (int64_t)gridDim.x * blockDim.x);
}

__global__ void dropout_bwd_kernel(const float* __restrict__ dy, const uint8_t* __restrict__ mask, float* __restrict__ dx,
                                   int64_t count, float keep) {
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < count; e += (int64_t)gridDim.x * blockDim.x)
        dx[e] = mask[e] ? dy[e] / keep : 0.f;
}

extern "C" int vl_dropout_fwd(const float* x, float* y, uint8_t* mask, int64_t count, float keep, uint64_t seed,
                              vl_stream_t stream) {
    VL_CHECK(x && y && mask && count > 0 && keep > 0.f && keep <= 1.f, "vl_dropout_fwd: bad argument");
    hipLaunchKernelGGL(dropout_fwd_kernel, dim3(grid_for(count, 256, 4096)), dim3(256), 0, (hipStream_t)stream, x, y, mask, count,
                       keep, seed);
    VL_LAUNCH_CHECK();
    return 0;
}

// the seed of vl_dropout_fwd as the engine forms it from its step count, read from the step state (a replayed step's own count)
__global__ void dropout_fwd_st_kernel(const float* __restrict__ x, float* __restrict__ y, uint8_t* __restrict__ mask, int64_t count,
                                      float keep, const vl_step_state* __restrict__ st) {
    dropout_fwd_body(x, y, mask, count, keep, ((uint64_t)st->step << 20) ^ 0x5DEECE66Dull, (int64_t)blockIdx.x * blockDim.x + threadIdx.x,
                     (int64_t)gridDim.x * blockDim.x);
}

extern "C" int vl_dropout_fwd_st(const float* x, float* y, uint8_t* mask, int64_t count, float keep, const vl_step_state* state,
                                 vl_stream_t stream) {
    VL_CHECK(x && y && mask && state && count > 0 && keep > 0.f && keep <= 1.f, "vl_dropout_fwd_st: bad argument");
    hipLaunchKernelGGL(dropout_fwd_st_kernel, dim3(grid_for(count, 256, 4096)), dim3(256), 0, (hipStream_t)stream, x, y, mask, count,
                       keep, state);
    VL_LAUNCH_CHECK();
    return 0;
}

extern "C" int vl_dropout_bwd(const float* dy, const uint8_t* mask, float* dx, int64_t count, float keep, vl_stream_t stream) {
    VL_CHECK(dy && dx && mask && count > 0 && keep > 0.f && keep <= 1.f, "vl_dropout_bwd: bad argument");
    hipLaunchKernelGGL(dropout_bwd_kernel, dim3(grid_for(count, 256, 4096)), dim3(256), 0, (hipStream_t)stream, dy, mask, dx, count,
                       keep);
    VL_LAUNCH_CHECK();
    return 0;
}

// ---- softmax cross-entropy, mean over the batch (train.py:120-123) + accuracy (142-149) --------
// One wave per row.  Row losses / hits go to a per-row workspace and are summed in a fixed order by a second one-workgroup
// kernel -> bitwise reproducible at any batch; without a workspace one workgroup walks all rows (small batches only).
// One row routine and one set of kernels serve every entry point, under two compile-time switches:
//   LS   label smoothing + top-k hits (vl_softmax_xent_ls): y' = y (1 - eps) + eps / C in place of y, per element (not the
//        algebraic form: at eps == 0 y' is y exactly and every sum is the plain one, bit for bit), one more lane-strided pass for the
//        label's rank among the logits (top_k == 0: no pass), a third workspace column and stats[2].
//   MIX  mixup / CutMix labels (vl_softmax_xent_mix; with LS): y' = lam y + (1 - lam) yp ahead of the smoothing, yp the
//        partner's label row.  At lam == 1 y' is y exactly (labels are small non-negative integers): the bits of LS alone.
//   WF   class weights + focal loss (vl_softmax_xent_wf; with LS, with or without MIX): with p = softmax(z), w the class
//        weights (NULL: ones) and m_c = (1 - p_c)^gamma,
//            loss = sum_c w_c y'_c m_c (-log p_c)
//            a_c  = w_c y'_c (m_c - gamma (1 - p_c)^(gamma - 1) p_c log p_c),   A = sum_c a_c,   dz_j = (p_j A - a_j) gscale
//        log p_c = z_c - lse and 1 - p_c = -expm1f(log p_c); the second term of a_c is 0 where 1 - p_c == 0 (its limit), so a saturated
//        row stays finite at every gamma.  The weights sit inside the class sum; the normaliser stays the caller's row count (gscale),
//        not sum w.  gamma == 0 (uniform over the launch): m = 1 exactly, no pow / expm1; a_c = w_c y'_c does not depend on z, so A is
//        summed beside the exponentials and reduced with them, and dz is written once.  gamma > 0: A needs lse first, so a_c is parked
//        in dz and a last pass turns it into dz (each lane rereads only what it wrote).  An element with w_c y'_c == 0 skips the pow.
// The switches are template parameters and not launch arguments: the plain launch holds neither the smoothing arithmetic nor a second
// label load, and writes two workspace columns and stats[0..1] only (an ls launch costs 1.12 x a plain one at 1344 x 1000); no launch
// without WF holds a weight load, a pow or the reduction of A.

// One element of a mixup blend, used by the label loop below and by every loop of both dtypes of vl_mixup_pairs: the rounding steps are
// spelled out (1 - lam by the caller, two products, one sum), so an element's bits do not depend on which loop reached it.
__device__ __forceinline__ float mix_elem(float a, float b, float lam, float oml) {
#pragma clang fp contract(off)
    return lam * a + oml * b;
}

// yp (MIX only): the partner's label row (nullptr: the row is its own partner and reads no other label row than its own).  The hits
// are counted against the row's OWN labels.  hitk (LS only): rank = #{c : z_c > z_t} + #{c < t : z_c == z_t}, t the first arg-max of
// the label row; a top-k hit iff rank < k.
template <bool LS, bool MIX, bool WF>
__device__ __forceinline__ void xent_row(const float* __restrict__ z, const int32_t* __restrict__ y, const int32_t* __restrict__ yp,
                                         float* __restrict__ dz, int C, float gscale, float eps, int top_k, float lam,
                                         const float* __restrict__ cw, float gamma, int lane, float& loss, float& hit, float& hitk) {
    float mx = -INFINITY;
    int am = 0x7fffffff;
    for (int c = lane; c < C; c += 64) {
        const float v = z[c];
        if (v > mx) {
            mx = v;
            am = c;
        }
    }
    const float gmx = wave_max(mx);
    // first index attaining the maximum
    int cand = (mx == gmx) ? am : 0x7fffffff;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) cand = min(cand, __shfl_xor(cand, o, 64));
    const bool focal = WF && gamma != 0.f;            // (uniform over the launch)
    float se = 0.f, A = 0.f;
    for (int c = lane; c < C; c += 64) {
        se += expf(z[c] - gmx);
        if constexpr (WF) {
            if (!focal && dz) {                       // A = sum_c w_c y'_c: the same y' as the label loop below forms, from the same words
                const int32_t* yq = yp ? yp : y;
                const float lam_r = yp ? lam : 1.0f;
                float ys = (float)y[c];
                if constexpr (MIX) ys = mix_elem(ys, (float)yq[c], lam_r, 1.0f - lam_r);
                if constexpr (LS) ys = ys * (1.0f - eps) + eps / (float)C;
                A += (cw ? cw[c] : 1.0f) * ys;
            }
        }
    }
    se = wave_sum(se);
    if constexpr (WF)
        if (!focal && dz) A = wave_sum(A);
    const float lse = logf(se) + gmx;
    const float on = 1.0f - eps, off = eps / (float)C;
    float l = 0.f;
    int ymax = -2147483647 - 1, yarg = 0x7fffffff;
    // MIX: no branch inside the loop: with one, the partner's load was issued only after the row's own had come back and the logit's
    // only after both -- three memory latencies per iteration in the place of one.  A row that is its own partner loads its own row
    // twice (the same addresses) under the weights 1 and 0, which give y exactly.
    const int32_t* yq = yp ? yp : y;
    const float lam_r = yp ? lam : 1.0f, oml = 1.0f - lam_r;
    for (int c = lane; c < C; c += 64) {
        const int yv = y[c];
        float ys = (float)yv;
        if constexpr (MIX) ys = mix_elem(ys, (float)yq[c], lam_r, oml);
        if constexpr (LS) ys = ys * on + off;
        if constexpr (!WF) l += ys * (lse - z[c]);
        if (yv > ymax) {
            ymax = yv;
            yarg = c;
        }
        if constexpr (!WF) {
            if (dz) dz[c] = (expf(z[c] - lse) - ys) * gscale;
        } else {
            const float wy = (cw ? cw[c] : 1.0f) * ys, lp = z[c] - lse;
            if (!focal) {
                l += wy * (lse - z[c]);
                if (dz) dz[c] = (expf(lp) * A - wy) * gscale;
            } else {
                float a = 0.f;
                if (wy != 0.f) {
                    const float q = fmaxf(-expm1f(lp), 0.f), m = powf(q, gamma);        // q = 1 - p, m = q^gamma
                    l += wy * m * (lse - z[c]);
                    a = wy * (m - (q > 0.f ? gamma * (m / q) * expf(lp) * lp : 0.f));
                }
                A += a;
                if (dz) dz[c] = a;                    // parked until A is known
            }
        }
    }
    l = wave_sum(l);
    if constexpr (WF) {
        if (focal && dz) {
            A = wave_sum(A);
            for (int c = lane; c < C; c += 64) dz[c] = (expf(z[c] - lse) * A - dz[c]) * gscale;
        }
    }
    int gy = ymax;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) gy = max(gy, __shfl_xor(gy, o, 64));
    int ycand = (ymax == gy) ? yarg : 0x7fffffff;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) ycand = min(ycand, __shfl_xor(ycand, o, 64));
    loss = l;
    hit = (cand == ycand) ? 1.f : 0.f;
    hitk = 0.f;
    if constexpr (LS) {
        if (top_k > 0) {                              // (uniform over the wave: every lane takes part in the shuffles)
            const int t = min(ycand, C - 1);          // (ycand < C unless every label is INT_MIN: never index past the row)
            const float zt = z[t];
            int rank = 0;
            for (int c = lane; c < C; c += 64) {
                const float v = z[c];
                rank += (v > zt || (v == zt && c < t)) ? 1 : 0;
            }
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) rank += __shfl_xor(rank, o, 64);
            hitk = rank < top_k ? 1.f : 0.f;
        }
    }
}

// seq_len (nullable) with T: row r = b T + t is live iff t < seq_len[b].  A dead row is not read: it adds nothing to the sums and its
// dlogits row is zeros (the reference's non_padding_index, dataset_.py:327-383).  MIX takes no lengths and makes no such test.
__device__ __forceinline__ bool xent_row_dead(const int32_t* __restrict__ seq_len, int T, int r) {
    return seq_len && (r % T) >= seq_len[r / T];
}

__device__ __forceinline__ void xent_zero_row(float* __restrict__ dz, int C, int lane) {
    if (dz)
        for (int c = lane; c < C; c += 64) dz[c] = 0.f;
}

// the label row of row b's partner: row b % rpc of clip clips - 1 - b / rpc (nullptr: b is its own partner)
__device__ __forceinline__ const int32_t* mix_partner_labels(const int32_t* __restrict__ labels, int b, int batch, int rpc, int C) {
    const int pr = (batch / rpc - 1 - b / rpc) * rpc + b % rpc;
    return pr == b ? nullptr : labels + (int64_t)pr * C;
}

// Both kernels take the same arguments but for stats / rows.  seq_len, T: !MIX only; rpc, lam_arg, lam_dev: MIX only (lam is read from
// lam_dev, when given, as the kernel runs: a captured step replays with the lambda the host wrote before the replay); eps, top_k: LS;
// cw (nullable, float[C], read as the kernel runs), gamma: WF only -- last, so the arguments of the launches without WF stay where they were.
// Without a workspace: wave w walks rows w, w + 4, ...; stats += ((w0 + w1) + w2) + w3 per column.
template <bool LS, bool MIX, bool WF>
__global__ void xent_kernel(const float* __restrict__ logits, const int32_t* __restrict__ labels, float* __restrict__ dlogits,
                            float* __restrict__ stats, int batch, int C, float gscale, const int32_t* __restrict__ seq_len, int T, int rpc,
                            float eps, int top_k, float lam_arg, const float* __restrict__ lam_dev, const float* __restrict__ cw,
                            float gamma) {
    __shared__ float sl[4], sc[4], sk[4];
    const float lam = MIX && lam_dev ? *lam_dev : lam_arg;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    float loss_acc = 0.f, corr_acc = 0.f, topk_acc = 0.f;
    for (int b = wv; b < batch; b += 4) {
        float* dz = dlogits ? dlogits + (int64_t)b * C : nullptr;
        float l, h, hk;
        if (!MIX && xent_row_dead(seq_len, T, b)) {
            xent_zero_row(dz, C, lane);
            continue;
        }
        xent_row<LS, MIX, WF>(logits + (int64_t)b * C, labels + (int64_t)b * C, MIX ? mix_partner_labels(labels, b, batch, rpc, C) : nullptr,
                          dz, C, gscale, eps, top_k, lam, cw, gamma, lane, l, h, hk);
        loss_acc += l;
        corr_acc += h;
        topk_acc += hk;
    }
    if (lane == 0) {
        sl[wv] = loss_acc;
        sc[wv] = corr_acc;
        if constexpr (LS) sk[wv] = topk_acc;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        stats[0] += sl[0] + sl[1] + sl[2] + sl[3];
        stats[1] += sc[0] + sc[1] + sc[2] + sc[3];
        if constexpr (LS)
            if (top_k > 0) stats[2] += sk[0] + sk[1] + sk[2] + sk[3];
    }
}

// With a workspace: row b's loss, hit and (LS) top-k hit to rows[b], rows[batch + b], rows[2 batch + b]; zeros for a dead row.
template <bool LS, bool MIX, bool WF>
__global__ void xent_rows_kernel(const float* __restrict__ logits, const int32_t* __restrict__ labels, float* __restrict__ dlogits,
                                 float* __restrict__ rows, int batch, int C, float gscale, const int32_t* __restrict__ seq_len, int T,
                                 int rpc, float eps, int top_k, float lam_arg, const float* __restrict__ lam_dev,
                                 const float* __restrict__ cw, float gamma) {
    const int lane = threadIdx.x & 63, b = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (b >= batch) return;
    const float lam = MIX && lam_dev ? *lam_dev : lam_arg;
    float* dz = dlogits ? dlogits + (int64_t)b * C : nullptr;
    float l = 0.f, h = 0.f, hk = 0.f;
    if (!MIX && xent_row_dead(seq_len, T, b))
        xent_zero_row(dz, C, lane);
    else
        xent_row<LS, MIX, WF>(logits + (int64_t)b * C, labels + (int64_t)b * C, MIX ? mix_partner_labels(labels, b, batch, rpc, C) : nullptr,
                          dz, C, gscale, eps, top_k, lam, cw, gamma, lane, l, h, hk);
    if (lane == 0) {
        rows[b] = l;
        rows[batch + b] = h;
        if constexpr (LS) rows[2 * (int64_t)batch + b] = hk;
    }
}

// rows[0..batch) losses, rows[batch..2 batch) hits, (LS) rows[2 batch..3 batch) top-k hits -> stats += their sums; thread t adds rows
// t, t+256, ... then a fixed tree.  The columns do not mix, so stats[0..1] have the same bits under LS; top_k == 0: stats[2] is not
// touched.
template <bool LS>
__global__ void xent_sum_kernel(const float* __restrict__ rows, float* __restrict__ stats, int batch, int top_k) {
    __shared__ float sl[256], sc[256], sk[256];
    float l = 0.f, h = 0.f, hk = 0.f;
    for (int b = threadIdx.x; b < batch; b += 256) {
        l += rows[b];
        h += rows[batch + b];
        if constexpr (LS) hk += rows[2 * (int64_t)batch + b];
    }
    sl[threadIdx.x] = l;
    sc[threadIdx.x] = h;
    if constexpr (LS) sk[threadIdx.x] = hk;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) {
            sl[threadIdx.x] += sl[threadIdx.x + s];
            sc[threadIdx.x] += sc[threadIdx.x + s];
            if constexpr (LS) sk[threadIdx.x] += sk[threadIdx.x + s];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        stats[0] += sl[0];
        stats[1] += sc[0];
        if constexpr (LS)
            if (top_k > 0) stats[2] += sk[0];
    }
}

// what a loss launch takes; an entry point sets what it has and leaves the rest at the values under which it is the identity
struct xent_args {
    const float* logits;
    const int32_t* labels;
    float *dlogits, *stats, *rows;
    int batch, classes;
    float grad_scale;
    const int32_t* seq_len = nullptr;
    int T = 1, rows_per_clip = 1;
    float smoothing = 0.f;
    int top_k = 0;
    float lam = 1.f;
    const float* lam_dev = nullptr;
    const float* class_weights = nullptr;
    float gamma = 0.f;
};

template <bool LS, bool MIX, bool WF = false>
static int xent_launch(xent_args a, vl_stream_t stream) {
    if (!a.seq_len) a.T = 1;
    if (!a.rows) {
        hipLaunchKernelGGL((xent_kernel<LS, MIX, WF>), dim3(1), dim3(256), 0, (hipStream_t)stream, a.logits, a.labels, a.dlogits, a.stats,
                           a.batch, a.classes, a.grad_scale, a.seq_len, a.T, a.rows_per_clip, a.smoothing, a.top_k, a.lam, a.lam_dev,
                           a.class_weights, a.gamma);
        VL_LAUNCH_CHECK();
        return 0;
    }
    hipLaunchKernelGGL((xent_rows_kernel<LS, MIX, WF>), dim3((a.batch + 3) / 4), dim3(256), 0, (hipStream_t)stream, a.logits, a.labels,
                       a.dlogits, a.rows, a.batch, a.classes, a.grad_scale, a.seq_len, a.T, a.rows_per_clip, a.smoothing, a.top_k, a.lam,
                       a.lam_dev, a.class_weights, a.gamma);
    VL_LAUNCH_CHECK();
    hipLaunchKernelGGL((xent_sum_kernel<LS>), dim3(1), dim3(256), 0, (hipStream_t)stream, a.rows, a.stats, a.batch, a.top_k);
    VL_LAUNCH_CHECK();
    return 0;
}

extern "C" int vl_softmax_xent(const float* logits, const int32_t* labels, float* dlogits, float* stats, float* rows, int batch,
                               int classes, float grad_scale, vl_stream_t stream) {
    VL_CHECK(logits && labels && stats && batch > 0 && classes > 0, "vl_softmax_xent: bad argument");
    return xent_launch<false, false>({logits, labels, dlogits, stats, rows, batch, classes, grad_scale}, stream);
}

extern "C" int vl_softmax_xent_len(const float* logits, const int32_t* labels, float* dlogits, float* stats, float* rows, int batch,
                                   int classes, float grad_scale, const int32_t* seq_len, int T, vl_stream_t stream) {
    VL_CHECK(logits && labels && stats && batch > 0 && classes > 0, "vl_softmax_xent_len: bad argument");
    VL_CHECK(!seq_len || (T > 0 && batch % T == 0), "vl_softmax_xent_len: batch (%d rows) is not whole sequences of T = %d", batch, T);
    return xent_launch<false, false>({logits, labels, dlogits, stats, rows, batch, classes, grad_scale, seq_len, T}, stream);
}

extern "C" int vl_softmax_xent_ls(const float* logits, const int32_t* labels, float* dlogits, float* stats, float* rows, int batch,
                                  int classes, float grad_scale, const int32_t* seq_len, int T, float smoothing, int top_k,
                                  vl_stream_t stream) {
    VL_CHECK(logits && labels && stats && batch > 0 && classes > 0, "vl_softmax_xent_ls: bad argument");
    VL_CHECK(!seq_len || (T > 0 && batch % T == 0), "vl_softmax_xent_ls: batch (%d rows) is not whole sequences of T = %d", batch, T);
    VL_CHECK(smoothing >= 0.f && smoothing < 1.f, "vl_softmax_xent_ls: smoothing must lie in [0, 1), got %g", (double)smoothing);
    VL_CHECK(top_k >= 0, "vl_softmax_xent_ls: top_k must be >= 0, got %d", top_k);
    return xent_launch<true, false>({logits, labels, dlogits, stats, rows, batch, classes, grad_scale, seq_len, T, 1, smoothing, top_k},
                                    stream);
}

extern "C" int vl_softmax_xent_mix(const float* logits, const int32_t* labels, float* dlogits, float* stats, float* rows, int batch,
                                   int classes, float grad_scale, int rows_per_clip, float smoothing, int top_k, float lam,
                                   const float* lam_dev, vl_stream_t stream) {
    VL_CHECK(logits && labels && stats && batch > 0 && classes > 0, "vl_softmax_xent_mix: bad argument");
    VL_CHECK(rows_per_clip > 0 && batch % rows_per_clip == 0, "vl_softmax_xent_mix: batch (%d rows) is not whole clips of %d rows", batch,
             rows_per_clip);
    VL_CHECK(smoothing >= 0.f && smoothing < 1.f, "vl_softmax_xent_mix: smoothing must lie in [0, 1), got %g", (double)smoothing);
    VL_CHECK(top_k >= 0, "vl_softmax_xent_mix: top_k must be >= 0, got %d", top_k);
    VL_CHECK(lam_dev || (lam >= 0.f && lam <= 1.f), "vl_softmax_xent_mix: lam must lie in [0, 1], got %g", (double)lam);
    return xent_launch<true, true>(
        {logits, labels, dlogits, stats, rows, batch, classes, grad_scale, nullptr, 1, rows_per_clip, smoothing, top_k, lam, lam_dev}, stream);
}

// Class weights and the focal loss on top of _ls / _mix.  rows_per_clip 1, lam 1 and no lam_dev: no partner row is read
// and seq_len may mask rows; otherwise the labels are mixed as in _mix, which takes no lengths.
extern "C" int vl_softmax_xent_wf(const float* logits, const int32_t* labels, float* dlogits, float* stats, float* rows, int batch,
                                  int classes, float grad_scale, const int32_t* seq_len, int T, int rows_per_clip, float smoothing,
                                  int top_k, float lam, const float* lam_dev, const float* class_weights, float gamma,
                                  vl_stream_t stream) {
    VL_CHECK(logits && labels && stats && batch > 0 && classes > 0, "vl_softmax_xent_wf: bad argument");
    VL_CHECK(!seq_len || (T > 0 && batch % T == 0), "vl_softmax_xent_wf: batch (%d rows) is not whole sequences of T = %d", batch, T);
    VL_CHECK(rows_per_clip > 0 && batch % rows_per_clip == 0, "vl_softmax_xent_wf: batch (%d rows) is not whole clips of %d rows", batch,
             rows_per_clip);
    VL_CHECK(smoothing >= 0.f && smoothing < 1.f, "vl_softmax_xent_wf: smoothing must lie in [0, 1), got %g", (double)smoothing);
    VL_CHECK(top_k >= 0, "vl_softmax_xent_wf: top_k must be >= 0, got %d", top_k);
    VL_CHECK(lam_dev || (lam >= 0.f && lam <= 1.f), "vl_softmax_xent_wf: lam must lie in [0, 1], got %g", (double)lam);
    VL_CHECK(gamma >= 0.f && gamma <= 3.0e38f, "vl_softmax_xent_wf: gamma must be finite and >= 0, got %g", (double)gamma);
    const bool mix = rows_per_clip > 1 || lam_dev || lam != 1.f;
    VL_CHECK(!(mix && seq_len), "vl_softmax_xent_wf: seq_len cannot be combined with mixed labels (rows_per_clip > 1 or a lambda)");
    const xent_args a = {logits, labels, dlogits, stats, rows, batch, classes, grad_scale, seq_len, T, rows_per_clip, smoothing, top_k, lam,
                         lam_dev, class_weights, gamma};
    return mix ? xent_launch<true, true, true>(a, stream) : xent_launch<true, false, true>(a, stream);
}

// ---- sigmoid cross-entropy for multi-label rows (vl_sigmoid_xent): independent sigmoids per class ----------------------
// The other loss family, beside the softmax one above and in its form: one wave per row, a per-row workspace summed in a fixed order by
// xent_sum_kernel<true> (three columns), a one-workgroup form without a workspace, no atomics, bitwise reproducible.  The classes of a row
// do not couple, so ONE lane-strided pass does everything: the first arg-max of the logits, the loss, the gradient and the exact-match test.
// Per element, z the logit, y the 0/1 label, yp the partner row's (MIX), q = cw[c] (NULL: 1):
//     t  = mix_elem(y, yp, lam)               (lam == 1 or a row that is its own partner: y exactly)
//     t  = t (1 - eps) + eps / 2              (tf.losses.sigmoid_cross_entropy's smoothing; eps == 0: t exactly)
//     e  = exp(-|z|),  sp = log1p(e),  -log p = max(-z, 0) + sp,  -log(1 - p) = max(z, 0) + sp
//     p and 1 - p are 1 / (1 + e) and e / (1 + e), in the order the sign of z says: neither is formed by a subtraction from 1
//   gamma == 0 (uniform over the launch, no exp of a power):
//     l = q t (-log p) + (1 - t) (-log(1 - p));   dl/dz = p (q t + 1 - t) - q t, summed as (1 - t) p - q t (1 - p)
//   gamma > 0 (Lin et al. 2017 in its sigmoid form, separable in the two terms, so soft labels are well defined):
//     l = q t (1 - p)^g (-log p) + (1 - t) p^g (-log(1 - p)),   (1 - p)^g = exp(g log(1 - p)),  p^g = exp(g log p)
//     dl/dz = q t (1 - p)^g (g p log p - (1 - p)) + (1 - t) p^g (p - g (1 - p) log(1 - p))
//   The limits relied on.  At z = +120: e = 0, sp = 0, log p = -0, p = 1, 1 - p = 0, log(1 - p) = -120: (1 - p)^g = exp(-120 g) is
//   finite (0 for a large g), g p log p = 0 and g (1 - p) log(1 - p) = g 0 (-120) = 0 -- no division and no log of 0 anywhere, so every
//   term is a product of finite factors; z = -120 is the mirror image.  A power that has underflowed to 0 drops its whole term
//   (x^g g log x -> 0: the power falls faster than g grows), so a gamma near float's range cannot pair 0 with inf.
// Row loss = (1 / C) sum_c l_c and dz = dl/dz * gscale / C: the logged loss is the element mean of Keras / torch / tf.losses, and the
// gradients are C times smaller than a softmax row's under the same gscale.
// hit: the first arg-max of the logits is a class with y_c > 0 (the row's OWN labels); exact: (z_c > 0) == (y_c > 0) for every class
// (z == 0 predicts negative; a row without labels is never a hit and is exact iff no logit is positive).
template <bool MIX>
__device__ __forceinline__ void sxent_row(const float* __restrict__ z, const int32_t* __restrict__ y, const int32_t* __restrict__ yp,
                                          float* __restrict__ dz, int C, float gs, float eps, float lam, const float* __restrict__ cw,
                                          float gamma, int lane, float& loss, float& hit, float& exact) {
    const bool focal = gamma != 0.f;                  // (uniform over the launch)
    const float on = 1.0f - eps, off = 0.5f * eps;
    const int32_t* yq = yp ? yp : y;                  // (no branch in the loop: see xent_row)
    const float lam_r = yp ? lam : 1.0f, oml = 1.0f - lam_r;
    float mx = -INFINITY, l = 0.f;
    int am = 0x7fffffff, bad = 0;
    for (int c = lane; c < C; c += 64) {
        const float v = z[c];
        const int yv = y[c];
        float t = (float)yv;
        if constexpr (MIX) t = mix_elem(t, (float)yq[c], lam_r, oml);
        t = __fmaf_rn(t, on, off);                    // (one rounding, spelled out: the same bits with and without MIX; eps == 0: t)
        if (v > mx) {
            mx = v;
            am = c;
        }
        bad += ((v > 0.f) != (yv > 0)) ? 1 : 0;
        const float e = expf(-fabsf(v)), sp = log1pf(e), r = 1.0f / (1.0f + e), er = e * r;
        const float p = v >= 0.f ? r : er, np = v >= 0.f ? er : r;                  // p, 1 - p
        const float nlp = fmaxf(-v, 0.f) + sp, nlq = fmaxf(v, 0.f) + sp;            // -log p, -log(1 - p)
        const float qt = (cw ? cw[c] : 1.0f) * t, ut = 1.0f - t;
        float g;
        if (!focal) {
            l += qt * nlp + ut * nlq;
            g = ut * p - qt * np;
        } else {
            const float m1 = expf(-gamma * nlq), m0 = expf(-gamma * nlp);           // (1 - p)^g, p^g
            l += qt * m1 * nlp + ut * m0 * nlq;
            const float g1 = m1 > 0.f ? m1 * (-gamma * p * nlp - np) : 0.f;
            const float g0 = m0 > 0.f ? m0 * (p + gamma * np * nlq) : 0.f;
            g = qt * g1 + ut * g0;
        }
        if (dz) dz[c] = g * gs;
    }
    const float gmx = wave_max(mx);
    int cand = (mx == gmx) ? am : 0x7fffffff;         // first index attaining the maximum
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) cand = min(cand, __shfl_xor(cand, o, 64));
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) bad += __shfl_xor(bad, o, 64);
    loss = wave_sum(l) / (float)C;
    hit = (cand < C && y[cand] > 0) ? 1.f : 0.f;      // (cand < C unless no logit compares above -inf: never index past the row)
    exact = bad == 0 ? 1.f : 0.f;
}

// The two kernels, as xent_kernel / xent_rows_kernel: seq_len, T: !MIX only; rpc, lam_arg, lam_dev: MIX only; gs = grad_scale / C.
template <bool MIX>
__global__ void sxent_kernel(const float* __restrict__ logits, const int32_t* __restrict__ labels, float* __restrict__ dlogits,
                             float* __restrict__ stats, int batch, int C, float gs, const int32_t* __restrict__ seq_len, int T, int rpc,
                             float eps, float lam_arg, const float* __restrict__ lam_dev, const float* __restrict__ cw, float gamma) {
    __shared__ float sl[4], sc[4], sk[4];
    const float lam = MIX && lam_dev ? *lam_dev : lam_arg;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    float loss_acc = 0.f, hit_acc = 0.f, exact_acc = 0.f;
    for (int b = wv; b < batch; b += 4) {
        float* dz = dlogits ? dlogits + (int64_t)b * C : nullptr;
        float l, h, ex;
        if (!MIX && xent_row_dead(seq_len, T, b)) {
            xent_zero_row(dz, C, lane);
            continue;
        }
        sxent_row<MIX>(logits + (int64_t)b * C, labels + (int64_t)b * C, MIX ? mix_partner_labels(labels, b, batch, rpc, C) : nullptr, dz,
                       C, gs, eps, lam, cw, gamma, lane, l, h, ex);
        loss_acc += l;
        hit_acc += h;
        exact_acc += ex;
    }
    if (lane == 0) {
        sl[wv] = loss_acc;
        sc[wv] = hit_acc;
        sk[wv] = exact_acc;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        stats[0] += sl[0] + sl[1] + sl[2] + sl[3];
        stats[1] += sc[0] + sc[1] + sc[2] + sc[3];
        stats[2] += sk[0] + sk[1] + sk[2] + sk[3];
    }
}

template <bool MIX>
__global__ void sxent_rows_kernel(const float* __restrict__ logits, const int32_t* __restrict__ labels, float* __restrict__ dlogits,
                                  float* __restrict__ rows, int batch, int C, float gs, const int32_t* __restrict__ seq_len, int T, int rpc,
                                  float eps, float lam_arg, const float* __restrict__ lam_dev, const float* __restrict__ cw, float gamma) {
    const int lane = threadIdx.x & 63, b = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (b >= batch) return;
    const float lam = MIX && lam_dev ? *lam_dev : lam_arg;
    float* dz = dlogits ? dlogits + (int64_t)b * C : nullptr;
    float l = 0.f, h = 0.f, ex = 0.f;
    if (!MIX && xent_row_dead(seq_len, T, b))
        xent_zero_row(dz, C, lane);
    else
        sxent_row<MIX>(logits + (int64_t)b * C, labels + (int64_t)b * C, MIX ? mix_partner_labels(labels, b, batch, rpc, C) : nullptr, dz,
                       C, gs, eps, lam, cw, gamma, lane, l, h, ex);
    if (lane == 0) {
        rows[b] = l;
        rows[batch + b] = h;
        rows[2 * (int64_t)batch + b] = ex;
    }
}

template <bool MIX>
static int sxent_launch(const float* logits, const int32_t* labels, float* dlogits, float* stats, float* rows, int batch, int classes,
                        float gs, const int32_t* seq_len, int T, int rows_per_clip, float smoothing, float lam, const float* lam_dev,
                        const float* pos_weights, float gamma, vl_stream_t stream) {
    if (!rows) {
        hipLaunchKernelGGL((sxent_kernel<MIX>), dim3(1), dim3(256), 0, (hipStream_t)stream, logits, labels, dlogits, stats, batch, classes,
                           gs, seq_len, T, rows_per_clip, smoothing, lam, lam_dev, pos_weights, gamma);
        VL_LAUNCH_CHECK();
        return 0;
    }
    hipLaunchKernelGGL((sxent_rows_kernel<MIX>), dim3((batch + 3) / 4), dim3(256), 0, (hipStream_t)stream, logits, labels, dlogits, rows,
                       batch, classes, gs, seq_len, T, rows_per_clip, smoothing, lam, lam_dev, pos_weights, gamma);
    VL_LAUNCH_CHECK();
    hipLaunchKernelGGL((xent_sum_kernel<true>), dim3(1), dim3(256), 0, (hipStream_t)stream, rows, stats, batch, 1);    // (1: all three columns)
    VL_LAUNCH_CHECK();
    return 0;
}

extern "C" int vl_sigmoid_xent(const float* logits, const int32_t* labels, float* dlogits, float* stats, float* rows, int batch,
                               int classes, float grad_scale, const int32_t* seq_len, int T, int rows_per_clip, float smoothing, float lam,
                               const float* lam_dev, const float* pos_weights, float gamma, vl_stream_t stream) {
    VL_CHECK(logits && labels && stats && batch > 0 && classes > 0, "vl_sigmoid_xent: bad argument");
    VL_CHECK(!seq_len || (T > 0 && batch % T == 0), "vl_sigmoid_xent: batch (%d rows) is not whole sequences of T = %d", batch, T);
    VL_CHECK(rows_per_clip > 0 && batch % rows_per_clip == 0, "vl_sigmoid_xent: batch (%d rows) is not whole clips of %d rows", batch,
             rows_per_clip);
    VL_CHECK(smoothing >= 0.f && smoothing < 1.f, "vl_sigmoid_xent: smoothing must lie in [0, 1), got %g", (double)smoothing);
    VL_CHECK(lam_dev || (lam >= 0.f && lam <= 1.f), "vl_sigmoid_xent: lam must lie in [0, 1], got %g", (double)lam);
    VL_CHECK(gamma >= 0.f && gamma <= 3.0e38f, "vl_sigmoid_xent: gamma must be finite and >= 0, got %g", (double)gamma);
    const bool mix = rows_per_clip > 1 || lam_dev || lam != 1.f;
    VL_CHECK(!(mix && seq_len), "vl_sigmoid_xent: seq_len cannot be combined with mixed labels (rows_per_clip > 1 or a lambda)");
    const float gs = grad_scale / (float)classes;
    if (!seq_len) T = 1;
    return mix ? sxent_launch<true>(logits, labels, dlogits, stats, rows, batch, classes, gs, nullptr, 1, rows_per_clip, smoothing, lam,
                                    lam_dev, pos_weights, gamma, stream)
               : sxent_launch<false>(logits, labels, dlogits, stats, rows, batch, classes, gs, seq_len, T, 1, smoothing, 1.f, nullptr,
                                     pos_weights, gamma, stream);
}

// ---- mixup (Zhang et al. 2018): the paired in-place blend of the clips (the loss on the mixed labels: xent_row<., MIX>) --
// Clip i is paired with clip clips - 1 - i.  lam comes from the launch arguments or, when lam_dev is given, from the device when the
// kernel runs (a captured step replays with the lambda the host wrote before the replay).  Every loop of both dtypes blends with
// mix_elem (above), so an element's bits do not depend on which loop reached it.
__device__ __forceinline__ float bf16_bits_to_f32(uint32_t h) { return __builtin_bit_cast(float, h << 16); }
__device__ __forceinline__ uint32_t f32_to_bf16_bits(float f) {      // round to nearest even (v_cvt_pk_bf16_f32)
    const __bf16 h = (__bf16)f;
    return (uint32_t)__builtin_bit_cast(uint16_t, h);
}
// one 32-bit word = two bf16: both halves of a and b blended in fp32, a' into wa and b' into wb
__device__ __forceinline__ void mix_word_bf16(uint32_t& wa, uint32_t& wb, float lam, float oml) {
    const float a0 = bf16_bits_to_f32(wa & 0xffffu), a1 = __builtin_bit_cast(float, wa & 0xffff0000u);
    const float b0 = bf16_bits_to_f32(wb & 0xffffu), b1 = __builtin_bit_cast(float, wb & 0xffff0000u);
    wa = f32_to_bf16_bits(mix_elem(a0, b0, lam, oml)) | (f32_to_bf16_bits(mix_elem(a1, b1, lam, oml)) << 16);
    wb = f32_to_bf16_bits(mix_elem(b0, a0, lam, oml)) | (f32_to_bf16_bits(mix_elem(b1, a1, lam, oml)) << 16);
}

// grid (x: the threads that walk one pair's elements, y: pairs).  A thread loads the same offset of both partners and writes both:
// the pairing is an involution, so nothing is read after it was written and no second buffer is needed.  The middle clip of an odd
// count belongs to no pair.  lam == 1 returns before any access: the identity holds for every bit pattern (-0, inf and NaN too).
// 16-byte accesses where both clip bases are 16-byte aligned (an odd elems misaligns every second clip: those pairs go element by
// element); the last elems % 4 floats of an aligned pair go element by element too.
__global__ void mixup_pairs_f32_kernel(float* __restrict__ x, int clips, int64_t elems, float lam_arg, const float* __restrict__ lam_dev) {
    const float lam = lam_dev ? *lam_dev : lam_arg;
    if (lam == 1.0f) return;
    const float oml = 1.0f - lam;
    const int64_t i0 = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, step = (int64_t)gridDim.x * blockDim.x;
    for (int j = blockIdx.y; j < clips / 2; j += gridDim.y) {
        float* __restrict__ a = x + (int64_t)j * elems;
        float* __restrict__ b = x + (int64_t)(clips - 1 - j) * elems;
        int64_t vec = 0;                                              // floats of the pair that go as 16-byte words
        if ((((uintptr_t)a | (uintptr_t)b) & 15) == 0) {              // (uniform over the workgroup)
            vec = elems & ~(int64_t)3;
            float4* __restrict__ a4 = reinterpret_cast<float4*>(a);
            float4* __restrict__ b4 = reinterpret_cast<float4*>(b);
            for (int64_t i = i0; i < vec / 4; i += step) {
                const float4 av = a4[i], bv = b4[i];
                a4[i] = make_float4(mix_elem(av.x, bv.x, lam, oml), mix_elem(av.y, bv.y, lam, oml), mix_elem(av.z, bv.z, lam, oml),
                                    mix_elem(av.w, bv.w, lam, oml));
                b4[i] = make_float4(mix_elem(bv.x, av.x, lam, oml), mix_elem(bv.y, av.y, lam, oml), mix_elem(bv.z, av.z, lam, oml),
                                    mix_elem(bv.w, av.w, lam, oml));
            }
        }
        for (int64_t i = vec + i0; i < elems; i += step) {
            const float av = a[i], bv = b[i];
            a[i] = mix_elem(av, bv, lam, oml);
            b[i] = mix_elem(bv, av, lam, oml);
        }
    }
}

// packed bf16: elems is a multiple of 8 (checked on the host), so every clip base is 16-byte aligned iff x is; else word by word
// (4-byte alignment is checked on the host)
__global__ void mixup_pairs_bf16_kernel(uint32_t* __restrict__ x, int clips, int64_t words, float lam_arg,
                                        const float* __restrict__ lam_dev) {
    const float lam = lam_dev ? *lam_dev : lam_arg;
    if (lam == 1.0f) return;
    const float oml = 1.0f - lam;
    const int64_t i0 = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, step = (int64_t)gridDim.x * blockDim.x;
    for (int j = blockIdx.y; j < clips / 2; j += gridDim.y) {
        uint32_t* __restrict__ a = x + (int64_t)j * words;
        uint32_t* __restrict__ b = x + (int64_t)(clips - 1 - j) * words;
        if ((((uintptr_t)a | (uintptr_t)b) & 15) == 0) {
            uint4* __restrict__ a4 = reinterpret_cast<uint4*>(a);
            uint4* __restrict__ b4 = reinterpret_cast<uint4*>(b);
            for (int64_t i = i0; i < words / 4; i += step) {
                uint4 av = a4[i], bv = b4[i];
                mix_word_bf16(av.x, bv.x, lam, oml);
                mix_word_bf16(av.y, bv.y, lam, oml);
                mix_word_bf16(av.z, bv.z, lam, oml);
                mix_word_bf16(av.w, bv.w, lam, oml);
                a4[i] = av;
                b4[i] = bv;
            }
        } else {
            for (int64_t i = i0; i < words; i += step) {
                uint32_t av = a[i], bv = b[i];
                mix_word_bf16(av, bv, lam, oml);
                a[i] = av;
                b[i] = bv;
            }
        }
    }
}

extern "C" int vl_mixup_pairs(void* x, int dtype, int clips, int64_t clip_elems, float lam, const float* lam_dev, vl_stream_t stream) {
    VL_CHECK(x, "vl_mixup_pairs: x is null");
    VL_CHECK(clips >= 0, "vl_mixup_pairs: clips must be >= 0, got %d", clips);
    VL_CHECK(clip_elems > 0, "vl_mixup_pairs: clip_elems must be > 0, got %lld", (long long)clip_elems);
    VL_CHECK(dtype == 0 || dtype == 1, "vl_mixup_pairs: dtype must be 0 (fp32) or 1 (packed bf16), got %d", dtype);
    VL_CHECK(dtype == 0 || clip_elems % 8 == 0, "vl_mixup_pairs: a packed-bf16 clip is whole 16-byte blocks: clip_elems %lld is no multiple of 8",
             (long long)clip_elems);
    VL_CHECK(lam_dev || (lam >= 0.f && lam <= 1.f), "vl_mixup_pairs: lam must lie in [0, 1], got %g", (double)lam);   // (NaN fails both)
    VL_CHECK(((uintptr_t)x & 3) == 0, "vl_mixup_pairs: x is not 4-byte aligned");
    if (clips <= 1) return 0;
    // pairs on grid y; per pair one thread per 4 16-byte words, so that a large clip is a few passes of a grid of at most 4096 workgroups
    const int pairs = clips / 2, gy = pairs < 4096 ? pairs : 4096;
    const int64_t words16 = (dtype == 0 ? clip_elems / 4 : clip_elems / 8) + 1;
    const dim3 grid(grid_for((words16 + 3) / 4, 256, 4096 / gy), gy);
    if (dtype == 0)
        hipLaunchKernelGGL(mixup_pairs_f32_kernel, grid, dim3(256), 0, (hipStream_t)stream, (float*)x, clips, clip_elems, lam, lam_dev);
    else
        hipLaunchKernelGGL(mixup_pairs_bf16_kernel, grid, dim3(256), 0, (hipStream_t)stream, (uint32_t*)x, clips, clip_elems / 2, lam,
                           lam_dev);
    VL_LAUNCH_CHECK();
    return 0;
}

// ---- CutMix / VideoMix (Yun et al. 2019, 2020): one (t, y, x) box swapped between the paired clips, in place, in x0 -----
// x0 is what input_prep_u8_kernel writes: [clips * fpc][3][phase][oh + 2 halo][wq] with logical pixel (y, x) of channel c in plane
// c * phase + (x + halo) % phase, row y + halo, column (x + halo) / phase.  In the plane of phase ph the box's columns are the
// contiguous run q in [ceil((x0 + halo - ph) / phase), ceil((x1 + halo - ph) / phase)).
// grid (x: tiles of CUT_ROWS rows, y: the frame of the clip, z: pairs), the same for every box; blockDim (64, 4).  A workgroup whose
// frame or rows lie outside the box returns after a uniform branch.  A wave takes one (plane, row) piece at a time, its lanes along the
// row; a thread loads the same offset of both partners and stores both (the pairing is an involution: nothing is read after it was
// written).  The words move as integers, so every bit pattern (-0, NaN payloads) arrives as it left.
#define CUT_ROWS 8
__global__ __launch_bounds__(256) void cutmix_pairs_f32_kernel(uint32_t* __restrict__ x, int clips, int fpc, int oh, int ow, int halo,
                                                               int phase, int wq, vl_cut_box arg, const int32_t* __restrict__ box_dev) {
    int b[6];
    if (!cut_box_get(arg, box_dev, fpc, oh, ow, b)) return;
    const int t = blockIdx.y;
    if (t < b[0] || t >= b[1]) return;
    const int ylo = max(b[2], (int)blockIdx.x * CUT_ROWS), yhi = min(b[3], ((int)blockIdx.x + 1) * CUT_ROWS);
    if (ylo >= yhi) return;
    const int64_t plane = (int64_t)(oh + 2 * halo) * wq, frame = 3 * phase * plane;
    const int lane = threadIdx.x, wv = __builtin_amdgcn_readfirstlane(threadIdx.y);
    for (int j = blockIdx.z; j < clips / 2; j += gridDim.z) {
        uint32_t* __restrict__ pa = x + ((int64_t)j * fpc + t) * frame;
        uint32_t* __restrict__ pb = x + ((int64_t)(clips - 1 - j) * fpc + t) * frame;
        for (int i = wv; i < 3 * phase * CUT_ROWS; i += 4) {
            const int pl = i / CUT_ROWS, y = ylo + i % CUT_ROWS, ph = pl % phase;
            if (y >= yhi) continue;
            const int qlo = (b[4] + halo - ph + phase - 1) / phase, qhi = (b[5] + halo - ph + phase - 1) / phase;
            const int64_t row = pl * plane + (int64_t)(y + halo) * wq;
            for (int q = qlo + lane; q < qhi; q += 64) {
                const uint32_t av = pa[row + q], bv = pb[row + q];
                pa[row + q] = bv;
                pb[row + q] = av;
            }
        }
    }
}

extern "C" int vl_cutmix_pairs(float* x0, int clips, int fpc, int out_h, int out_w, int halo, int phase, const int32_t* box_host,
                               const int32_t* box_dev, vl_stream_t stream) {
    VL_CHECK(x0, "vl_cutmix_pairs: x0 is null");
    VL_CHECK(box_host || box_dev, "vl_cutmix_pairs: both box pointers are null");
    VL_CHECK(clips >= 0, "vl_cutmix_pairs: clips must be >= 0, got %d", clips);
    VL_CHECK(fpc > 0 && fpc <= 65535, "vl_cutmix_pairs: fpc must lie in [1, 65535], got %d", fpc);
    VL_CHECK(out_h > 0 && out_w > 0, "vl_cutmix_pairs: bad frame size %d x %d", out_h, out_w);
    VL_CHECK(halo >= 0, "vl_cutmix_pairs: halo must be >= 0, got %d", halo);
    VL_CHECK(phase >= 1, "vl_cutmix_pairs: phase must be >= 1, got %d", phase);
    VL_CHECK(((uintptr_t)x0 & 3) == 0, "vl_cutmix_pairs: x0 is not 4-byte aligned");
    vl_cut_box box = {{0, 0, 0, 0, 0, 0}};
    if (!box_dev) {
        if (int rc = cut_box_host_check(box_host, fpc, out_h, out_w, "vl_cutmix_pairs", &box)) return rc;
        if (box.v[0] == box.v[1] || box.v[2] == box.v[3] || box.v[4] == box.v[5]) return 0;
    }
    if (clips <= 1) return 0;
    const int wq = (out_w + 2 * halo + phase - 1) / phase, pairs = clips / 2;
    const dim3 grid((out_h + CUT_ROWS - 1) / CUT_ROWS, fpc, pairs < 65535 ? pairs : 65535);
    hipLaunchKernelGGL(cutmix_pairs_f32_kernel, grid, dim3(64, 4), 0, (hipStream_t)stream, (uint32_t*)x0, clips, fpc, out_h, out_w, halo,
                       phase, wq, box, box_dev);
    VL_LAUNCH_CHECK();
    return 0;
}

// ---- random erasing (Zhong et al. 2017): every clip's own (t, y, x) box overwritten in place, in x0 ---------------------
// The layout and the column runs are those of the CutMix kernel above; the launch is write-only and per clip.  A clip's box and key
// come from its row of the device table (erase_row_get, common.h) when the kernel runs.  grid (x: tiles of CUT_ROWS rows, y: the
// frame of the clip, z: clips), the same for every table; a workgroup whose frame or rows lie outside a clip's box goes on to its next
// clip after a uniform branch.  mode 0 stores +0, mode 1 one value per (clip, channel), mode 2 a value per element from its LOGICAL
// index ((t 3 + c) oh + y) ow + x, so that the packed form (vl_erase_boxes_s2d) draws the same value for the same pixel.
__global__ __launch_bounds__(256) void erase_boxes_f32_kernel(float* __restrict__ x, int clips, int fpc, int oh, int ow, int halo, int phase,
                                                              int wq, const int32_t* __restrict__ table, int mode, float scale) {
    const int t = blockIdx.y;
    const int64_t plane = (int64_t)(oh + 2 * halo) * wq, frame = 3 * phase * plane;
    const int lane = threadIdx.x, wv = __builtin_amdgcn_readfirstlane(threadIdx.y);
    for (int j = blockIdx.z; j < clips; j += gridDim.z) {
        int b[6];
        uint64_t key;
        if (!erase_row_get(table + (int64_t)j * ERASE_ROW_WORDS, fpc, oh, ow, b, key)) continue;
        if (t < b[0] || t >= b[1]) continue;
        const int ylo = max(b[2], (int)blockIdx.x * CUT_ROWS), yhi = min(b[3], ((int)blockIdx.x + 1) * CUT_ROWS);
        if (ylo >= yhi) continue;
        float* __restrict__ p = x + ((int64_t)j * fpc + t) * frame;
        float cv[3] = {0.f, 0.f, 0.f};               // mode 1: the clip's three channel values, once per workgroup
        if (mode == 1) {                             // lanes 0 .. 2 hash one channel each, then every lane reads the three
            const float mine = erase_noise(key, ERASE_CLIP_ELEMENT + (uint64_t)(lane < 3 ? lane : 0), scale);
#pragma unroll
            for (int c = 0; c < 3; ++c) cv[c] = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, mine), c));
        }
        // the column run of a phase is formed once (two divisions); then a wave takes one (channel, row) piece of it at a time, with a
        // few multiplies of index arithmetic per piece
        for (int ph = 0; ph < phase; ++ph) {
            const int qlo = (b[4] + halo - ph + phase - 1) / phase, qhi = (b[5] + halo - ph + phase - 1) / phase;
            if (qlo >= qhi) continue;
            for (int i = wv; i < 3 * CUT_ROWS; i += 4) {
                const int c = i / CUT_ROWS, y = ylo + i % CUT_ROWS;
                if (y >= yhi) continue;
                const int64_t row = (int64_t)(c * phase + ph) * plane + (int64_t)(y + halo) * wq;
                const uint64_t e0 = ((uint64_t)(t * 3 + c) * oh + y) * ow;
                float v = c == 0 ? cv[0] : (c == 1 ? cv[1] : cv[2]);
                for (int q = qlo + lane; q < qhi; q += 64) {
                    if (mode == 2) v = erase_noise(key, e0 + (uint64_t)(q * phase + ph - halo), scale);
                    p[row + q] = v;
                }
            }
        }
    }
}

extern "C" int vl_erase_boxes(float* x0, int clips, int fpc, int out_h, int out_w, int halo, int phase, const int32_t* table_dev, int mode,
                              float scale, vl_stream_t stream) {
    VL_CHECK(x0, "vl_erase_boxes: x0 is null");
    VL_CHECK(table_dev, "vl_erase_boxes: table_dev is null");
    VL_CHECK(clips >= 0, "vl_erase_boxes: clips must be >= 0, got %d", clips);
    VL_CHECK(fpc > 0 && fpc <= 65535, "vl_erase_boxes: fpc must lie in [1, 65535], got %d", fpc);
    VL_CHECK(out_h > 0 && out_w > 0, "vl_erase_boxes: bad frame size %d x %d", out_h, out_w);
    VL_CHECK(halo >= 0, "vl_erase_boxes: halo must be >= 0, got %d", halo);
    VL_CHECK(phase >= 1, "vl_erase_boxes: phase must be >= 1, got %d", phase);
    VL_CHECK(mode >= 0 && mode <= 2, "vl_erase_boxes: mode must be 0 (zero), 1 (clip) or 2 (pixel), got %d", mode);
    VL_CHECK(erase_scale_ok(scale), "vl_erase_boxes: scale must be finite");
    VL_CHECK(((uintptr_t)x0 & 3) == 0 && ((uintptr_t)table_dev & 3) == 0, "vl_erase_boxes: x0 / table_dev is not 4-byte aligned");
    if (clips == 0) return 0;
    const int wq = (out_w + 2 * halo + phase - 1) / phase;
    const dim3 grid((out_h + CUT_ROWS - 1) / CUT_ROWS, fpc, clips < 65535 ? clips : 65535);
    hipLaunchKernelGGL(erase_boxes_f32_kernel, grid, dim3(64, 4), 0, (hipStream_t)stream, x0, clips, fpc, out_h, out_w, halo, phase, wq,
                       table_dev, mode, scale);
    VL_LAUNCH_CHECK();
    return 0;
}

// ---- global norm + SGD / Adam (train.py:199-222) ----------------------------------------------
// ---- tier table (vltf.h: vl_lr_tier): the ranges of the flat buffer an update / a norm touches, by value in the launch arguments --
struct tier_table {
    vl_lr_tier t[VL_MAX_LR_TIERS];
    int n;
};

// The rules every range table keeps (tier, decay, LARS and LAMB tables alike; the kernels rely on them: an element outside every range
// is never addressed, and no element is addressed twice).  An entry is named `open`k`close` in the messages: "tier 2", "ranges[2]".
// Entry k begins at or after `prev` (its predecessor's end), is not empty and ends inside [0, count); count < 0: the bound is not known.
static int range_bounds_check(const char* who, const char* open, int k, const char* close, int64_t begin, int64_t end, int64_t prev,
                              int64_t count) {
    VL_CHECK(begin >= prev && end > begin && (count < 0 || end <= count),
             "%s: %s%d%s = [%lld, %lld) is empty, unsorted, overlaps its predecessor or leaves [0, %lld)", who, open, k, close,
             (long long)begin, (long long)end, (long long)count);
    return 0;
}
// a multiplier is finite and > 0, a decay finite and >= 0 (NaN fails both comparisons)
static int range_factor_check(const char* who, const char* open, int k, const char* close, const char* name, float x, bool positive) {
    VL_CHECK((positive ? x > 0.f : x >= 0.f) && x <= 3.402823466e38f, "%s: %s%d%s: %s must be finite and %s", who, open, k, close, name,
             positive ? "> 0" : ">= 0");
    return 0;
}

static tier_table tier_table_full(int64_t count) {
    tier_table tt;
    tt.t[0].begin = 0;
    tt.t[0].end = count;
    tt.t[0].lr_mult = 1.f;
    tt.n = 1;
    return tt;
}

// null_is_full: a NULL table of 0 entries is the full range (vl_momentum_apply, vl_grad_accumulate, vl_ema_update)
static int tier_table_make(const char* who, const vl_lr_tier* tiers, int n_tiers, int64_t count, tier_table* out, bool null_is_full = false) {
    if (null_is_full && !tiers && n_tiers == 0) {
        *out = tier_table_full(count);
        return 0;
    }
    VL_CHECK(tiers && n_tiers >= 1 && n_tiers <= VL_MAX_LR_TIERS, "%s: 1 .. %d tiers, got %d", who, VL_MAX_LR_TIERS, n_tiers);
    int64_t prev = 0;
    for (int k = 0; k < n_tiers; ++k) {
        const vl_lr_tier& t = tiers[k];
        if (int rc = range_bounds_check(who, "tier ", k, "", t.begin, t.end, prev, count)) return rc;
        if (int rc = range_factor_check(who, "tier ", k, "", "lr_mult", t.lr_mult, true)) return rc;
        out->t[k] = t;
        prev = t.end;
    }
    out->n = n_tiers;
    return 0;
}

// [begin, end) = scalar head [begin, v0) + 16-byte interior [v0, v1) + scalar tail [v1, end).  The interior exists where every one of the
// arrays is 16-byte aligned at the same element: `phase` = (address / 4) mod 4 of element 0, < 0 when the arrays disagree.
__device__ __forceinline__ int align_phase(const void* a, const void* b, const void* c, const void* d) {
    const int pa = (int)(((uintptr_t)a >> 2) & 3);
    const bool same = (!b || (int)(((uintptr_t)b >> 2) & 3) == pa) && (!c || (int)(((uintptr_t)c >> 2) & 3) == pa) &&
                      (!d || (int)(((uintptr_t)d >> 2) & 3) == pa);
    return same ? pa : -1;
}
__device__ __forceinline__ void tier_split(int64_t begin, int64_t end, int phase, int64_t& v0, int64_t& v1) {
    if (phase < 0) {
        v0 = v1 = end;
        return;
    }
    v0 = begin + ((4 - (int)((begin + phase) & 3)) & 3);
    if (v0 > end) v0 = end;
    v1 = v0 + ((end - v0) & ~(int64_t)3);
}
// The one walk of a range, for a lane that starts at i0 and strides by `step`: f1(i) for element i of the head and of the tail, f4(v0, i)
// for 16-byte vector i of the interior, whose vector 0 begins at element v0.  Every ranged kernel below goes through here, so which
// elements a range addresses, and which loop reaches each, is stated once; f1 and f4 share an element function, so an element's result
// does not depend on the loop that reached it.
template <class F1, class F4>
__device__ __forceinline__ void range_walk(int64_t begin, int64_t end, int phase, int64_t i0, int64_t step, F1 f1, F4 f4) {
    int64_t v0, v1;
    tier_split(begin, end, phase, v0, v1);
    for (int64_t i = begin + i0; i < v0; i += step) f1(i);
    for (int64_t i = i0; i < (v1 - v0) / 4; i += step) f4(v0, i);
    for (int64_t i = v1 + i0; i < end; i += step) f1(i);
}
// 16-byte vector i counted from element v0 of p.  (One element offset on purpose: as `((float4*)(p + v0))[i]` hipcc keeps a pointer per
// array through the interiors of grad_accumulate_kernel and l2_regularize_stage1, one more 64-bit add per pass: DESIGN.md 4.4.)
__device__ __forceinline__ float4& vec4(float* p, int64_t v0, int64_t i) { return *reinterpret_cast<float4*>(p + v0 + 4 * i); }
__device__ __forceinline__ const float4& vec4(const float* p, int64_t v0, int64_t i) { return *reinterpret_cast<const float4*>(p + v0 + 4 * i); }

__global__ void sumsq_stage1(const float* __restrict__ g, int64_t count, float* __restrict__ ws) {
    __shared__ float sm[4];
    float acc = 0.f;
    const int64_t nvec = count / 4;
    const float4* g4 = reinterpret_cast<const float4*>(g);
    const bool aligned = ((uintptr_t)g & 15) == 0;
    if (aligned) {
        for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < nvec; i += (int64_t)gridDim.x * blockDim.x) {
            const float4 v = g4[i];
            acc += v.x * v.x + v.y * v.y + v.z * v.z + v.w * v.w;
        }
        for (int64_t i = nvec * 4 + (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < count; i += (int64_t)gridDim.x * blockDim.x)
            acc += g[i] * g[i];
    } else {
        for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < count; i += (int64_t)gridDim.x * blockDim.x)
            acc += g[i] * g[i];
    }
    acc = block_sum_256(acc, sm);
    if (threadIdx.x == 0) ws[blockIdx.x] = acc;
}

__global__ void sumsq_stage2(const float* __restrict__ ws, int nblocks, float* __restrict__ out, int accumulate) {
    __shared__ float sm[4];
    float acc = 0.f;
    for (int i = threadIdx.x; i < nblocks; i += 256) acc += ws[i];
    acc = block_sum_256(acc, sm);
    if (threadIdx.x == 0) out[0] = accumulate ? out[0] + acc : acc;
}

extern "C" int vl_sumsq(const float* g, int64_t count, float* out, float* ws, int accumulate, vl_stream_t stream) {
    VL_CHECK(g && out && ws && count > 0, "vl_sumsq: bad argument");
    const int blocks = grid_for(count / 4 + 1, 256, 1024);
    hipLaunchKernelGGL(sumsq_stage1, dim3(blocks), dim3(256), 0, (hipStream_t)stream, g, count, ws);
    VL_LAUNCH_CHECK();
    hipLaunchKernelGGL(sumsq_stage2, dim3(1), dim3(256), 0, (hipStream_t)stream, ws, blocks, out, accumulate);
    VL_LAUNCH_CHECK();
    return 0;
}

// vl_sumsq over the elements inside the tiers only (the multipliers play no part).  A lane walks the tiers in table order -- head,
// 16-byte interior, tail of each -- so the order of every partial sum is fixed by the table and the grid.
__global__ void sumsq_tiers_stage1(const float* __restrict__ g, tier_table tt, float* __restrict__ ws) {
    __shared__ float sm[4];
    float acc = 0.f;
    const int64_t i0 = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, step = (int64_t)gridDim.x * blockDim.x;
    const int phase = align_phase(g, nullptr, nullptr, nullptr);
    for (int k = 0; k < tt.n; ++k)
        range_walk(tt.t[k].begin, tt.t[k].end, phase, i0, step, [&](int64_t i) { acc += g[i] * g[i]; },
                   [&](int64_t v0, int64_t i) {
                       const float4 v = vec4(g, v0, i);
                       acc += v.x * v.x + v.y * v.y + v.z * v.z + v.w * v.w;
                   });
    acc = block_sum_256(acc, sm);
    if (threadIdx.x == 0) ws[blockIdx.x] = acc;
}

extern "C" int vl_sumsq_tiers(const float* g, int64_t count, const vl_lr_tier* tiers, int n_tiers, float* out, float* ws, vl_stream_t stream) {
    VL_CHECK(g && out && ws && count > 0, "vl_sumsq_tiers: bad argument");
    tier_table tt;
    if (int rc = tier_table_make("vl_sumsq_tiers", tiers, n_tiers, count, &tt)) return rc;
    int64_t inside = 0;
    for (int k = 0; k < tt.n; ++k) inside += tt.t[k].end - tt.t[k].begin;
    const int blocks = grid_for(inside / 4 + 1, 256, 1024);
    hipLaunchKernelGGL(sumsq_tiers_stage1, dim3(blocks), dim3(256), 0, (hipStream_t)stream, g, tt, ws);
    VL_LAUNCH_CHECK();
    hipLaunchKernelGGL(sumsq_stage2, dim3(1), dim3(256), 0, (hipStream_t)stream, ws, blocks, out, 0);
    VL_LAUNCH_CHECK();
    return 0;
}

// ---- L2 weight decay fused into the norm launch (vltf.h: vl_l2_regularize) ----------------------------------------------------------
// g <- g + decay w in place, then the two sums of the regularised gradient and of the regulariser.  The table travels by value like
// the tier table; a range with decay 0 (biases) is vl_sumsq_tiers' loop: g read once, w never loaded, g never stored.
struct decay_table {
    vl_decay_range r[VL_MAX_DECAY_RANGES];
    int n;
};

static int decay_table_make(const char* who, const vl_decay_range* ranges, int n_ranges, int64_t count, decay_table* out) {
    VL_CHECK(ranges && n_ranges >= 1 && n_ranges <= VL_MAX_DECAY_RANGES, "%s: 1 .. %d ranges, got %d", who, VL_MAX_DECAY_RANGES, n_ranges);
    int64_t prev = 0;
    for (int k = 0; k < n_ranges; ++k) {
        const vl_decay_range& r = ranges[k];
        if (int rc = range_bounds_check(who, "range ", k, "", r.begin, r.end, prev, count)) return rc;
        if (int rc = range_factor_check(who, "range ", k, "", "decay", r.decay, false)) return rc;
        out->r[k] = r;
        prev = r.end;
    }
    out->n = n_ranges;
    return 0;
}

// one element function for the scalar and the 16-byte loops: an element's g' does not depend on the loop that reached it
__device__ __forceinline__ void l2_elem(float w, float& g, float decay, float half_decay, float& ss, float& rs) {
#pragma clang fp contract(off)
    const float gi = __builtin_fmaf(decay, w, g);
    g = gi;
    ss = ss + gi * gi;
    rs = rs + (half_decay * w) * w;
}
__device__ __forceinline__ void l2_elem4(const float4& w, float4& g, float decay, float half_decay, float& ss, float& rs) {
    l2_elem(w.x, g.x, decay, half_decay, ss, rs);
    l2_elem(w.y, g.y, decay, half_decay, ss, rs);
    l2_elem(w.z, g.z, decay, half_decay, ss, rs);
    l2_elem(w.w, g.w, decay, half_decay, ss, rs);
}

// ws[block] = the block's sum of g'^2, ws[1024 + block] = its sum of (decay / 2) w^2.  A lane walks the ranges in table order -- head,
// 16-byte interior, tail of each -- so every partial sum's order is fixed by the table and the grid (sumsq_tiers_stage1).  (Measured
// and dropped: two and four grid strides per pass of the interior with all loads issued first -- 106 and 109 us against 105 us for
// this loop on 44.6 M floats)
__global__ __launch_bounds__(256) void l2_regularize_stage1(const float* __restrict__ w, float* __restrict__ g, decay_table dt,
                                                            float* __restrict__ ws) {
    __shared__ float sm[4];
    float ss = 0.f, rs = 0.f;
    const int64_t i0 = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, step = (int64_t)gridDim.x * blockDim.x;
    const int phase = align_phase(w, g, nullptr, nullptr);
    for (int k = 0; k < dt.n; ++k) {
        const int64_t begin = dt.r[k].begin, end = dt.r[k].end;
        const float decay = dt.r[k].decay, half_decay = 0.5f * decay;
        if (decay > 0.f) {
            range_walk(begin, end, phase, i0, step,
                       [&](int64_t i) {
                           float gi = g[i];
                           l2_elem(w[i], gi, decay, half_decay, ss, rs);
                           g[i] = gi;
                       },
                       [&](int64_t v0, int64_t i) {
                           const float4 wv = vec4(w, v0, i);
                           float4 gv = vec4(g, v0, i);
                           l2_elem4(wv, gv, decay, half_decay, ss, rs);
                           vec4(g, v0, i) = gv;
                       });
        } else {                              // a read-only sum: w is never loaded, g never stored
            range_walk(begin, end, phase, i0, step, [&](int64_t i) { ss += g[i] * g[i]; },
                       [&](int64_t v0, int64_t i) {
                           const float4 v = vec4(g, v0, i);
                           ss += v.x * v.x + v.y * v.y + v.z * v.z + v.w * v.w;
                       });
        }
    }
    ss = block_sum_256(ss, sm);
    rs = block_sum_256(rs, sm);
    if (threadIdx.x == 0) {
        ws[blockIdx.x] = ss;
        ws[1024 + blockIdx.x] = rs;
    }
}

__global__ __launch_bounds__(256) void l2_regularize_stage2(const float* __restrict__ ws, int nblocks, float* __restrict__ out) {
    __shared__ float sm[4];
    float ss = 0.f, rs = 0.f;
    for (int i = threadIdx.x; i < nblocks; i += 256) {
        ss += ws[i];
        rs += ws[1024 + i];
    }
    ss = block_sum_256(ss, sm);
    rs = block_sum_256(rs, sm);
    if (threadIdx.x == 0) {
        out[0] = ss;
        out[1] = rs;
    }
}

extern "C" int vl_l2_regularize(const float* w, float* g, int64_t count, const vl_decay_range* ranges, int n_ranges, float* out, float* ws,
                                vl_stream_t stream) {
    VL_CHECK(w && g && out && ws && count > 0, "vl_l2_regularize: bad argument");
    decay_table dt;
    if (int rc = decay_table_make("vl_l2_regularize", ranges, n_ranges, count, &dt)) return rc;
    int64_t inside = 0;
    for (int k = 0; k < dt.n; ++k) inside += dt.r[k].end - dt.r[k].begin;
    const int blocks = grid_for(inside / 4 + 1, 256, 1024);
    hipLaunchKernelGGL(l2_regularize_stage1, dim3(blocks), dim3(256), 0, (hipStream_t)stream, w, g, dt, ws);
    VL_LAUNCH_CHECK();
    hipLaunchKernelGGL(l2_regularize_stage2, dim3(1), dim3(256), 0, (hipStream_t)stream, ws, blocks, out);
    VL_LAUNCH_CHECK();
    return 0;
}

__device__ __forceinline__ float clip_scale(float clip_norm, const float* sumsq, float gscale) {
    if (clip_norm <= 0.f || !sumsq) return gscale;
    const float norm = gscale * sqrtf(sumsq[0]);
    return gscale * clip_norm / fmaxf(norm, clip_norm);
}

// the update bodies (grid-stride start and step from the kernel, as dropout_fwd_body).  One element function each, used by the scalar
// and the 16-byte callable of range_walk alike: an element's result does not depend on which loop reached it.
// The rounding steps are spelled out (no contraction left to the compiler, which chose differently per loop): the forms are the
// ones the one-loop kernels were built with, so every loop here -- and the plain entry points before there were tiers -- give the same bits.
__device__ __forceinline__ float sgd_elem(float w, float g, float a) {
#pragma clang fp contract(off)
    return __builtin_fmaf(-a, g, w);
}

__device__ __forceinline__ void sgd_apply_body(float* __restrict__ w, const float* __restrict__ g, const tier_table& tt, float lr, float clip_norm,
                                               const float* __restrict__ sumsq, float gscale, int64_t i0, int64_t step) {
    const float sc = clip_scale(clip_norm, sumsq, gscale);
    const int phase = align_phase(w, g, nullptr, nullptr);
    for (int k = 0; k < tt.n; ++k) {
        const float a = (lr * tt.t[k].lr_mult) * sc;
        range_walk(tt.t[k].begin, tt.t[k].end, phase, i0, step, [&](int64_t i) { w[i] = sgd_elem(w[i], g[i], a); },
                   [&](int64_t v0, int64_t i) {
                       float4 wv = vec4(w, v0, i);
                       const float4 gv = vec4(g, v0, i);
                       wv.x = sgd_elem(wv.x, gv.x, a);
                       wv.y = sgd_elem(wv.y, gv.y, a);
                       wv.z = sgd_elem(wv.z, gv.z, a);
                       wv.w = sgd_elem(wv.w, gv.w, a);
                       vec4(w, v0, i) = wv;
                   });
    }
}

__device__ __forceinline__ void adam_elem(float& w, float g, float& m, float& v, float sc, float lr_t) {
#pragma clang fp contract(off)
    const float gi = g * sc;
    const float mi = __builtin_fmaf(0.9f, m, 0.1f * gi);
    const float vi = __builtin_fmaf(0.999f, v, gi * (0.001f * gi));
    m = mi;
    v = vi;
    w = w - (lr_t * mi) / (sqrtf(vi) + 1e-8f);
}

__device__ __forceinline__ void adam_apply_body(float* __restrict__ w, const float* __restrict__ g, float* __restrict__ m, float* __restrict__ v,
                                                const tier_table& tt, float lr_t, float clip_norm, const float* __restrict__ sumsq, float gscale,
                                                int64_t i0, int64_t step) {
    const float sc = clip_scale(clip_norm, sumsq, gscale);
    const int phase = align_phase(w, g, m, v);
    for (int k = 0; k < tt.n; ++k) {
        const float lr_k = lr_t * tt.t[k].lr_mult;
        range_walk(tt.t[k].begin, tt.t[k].end, phase, i0, step, [&](int64_t i) { adam_elem(w[i], g[i], m[i], v[i], sc, lr_k); },
                   [&](int64_t v0, int64_t i) {
                       float4 wv = vec4(w, v0, i), mv = vec4(m, v0, i), qv = vec4(v, v0, i);
                       const float4 gv = vec4(g, v0, i);
                       adam_elem(wv.x, gv.x, mv.x, qv.x, sc, lr_k);
                       adam_elem(wv.y, gv.y, mv.y, qv.y, sc, lr_k);
                       adam_elem(wv.z, gv.z, mv.z, qv.z, sc, lr_k);
                       adam_elem(wv.w, gv.w, mv.w, qv.w, sc, lr_k);
                       vec4(m, v0, i) = mv;
                       vec4(v, v0, i) = qv;
                       vec4(w, v0, i) = wv;
                   });
    }
}

// tf.train.MomentumOptimizer: the accumulator takes the clipped gradient, lr stays outside it (vltf.h: vl_momentum_apply)
__device__ __forceinline__ void momentum_elem(float& w, float g, float& a, float sc, float lr_k, float momentum, bool nesterov) {
#pragma clang fp contract(off)
    const float gi = g * sc;
    const float ai = __builtin_fmaf(momentum, a, gi);
    a = ai;
    w = __builtin_fmaf(-lr_k, nesterov ? __builtin_fmaf(momentum, ai, gi) : ai, w);
}

// one range [begin, end) of the momentum update with its own lr_k (range_walk).  Shared by the tier walk below and by the LARS walk
// (lars_apply_body), so a range's bits do not depend on which table named it.
__device__ __forceinline__ void momentum_range(float* __restrict__ w, const float* __restrict__ g, float* __restrict__ a, int64_t begin,
                                               int64_t end, int phase, float sc, float lr_k, float momentum, bool nesterov, int64_t i0,
                                               int64_t step) {
    range_walk(begin, end, phase, i0, step, [&](int64_t i) { momentum_elem(w[i], g[i], a[i], sc, lr_k, momentum, nesterov); },
               [&](int64_t v0, int64_t i) {
                   float4 wv = vec4(w, v0, i), av = vec4(a, v0, i);
                   const float4 gv = vec4(g, v0, i);
                   momentum_elem(wv.x, gv.x, av.x, sc, lr_k, momentum, nesterov);
                   momentum_elem(wv.y, gv.y, av.y, sc, lr_k, momentum, nesterov);
                   momentum_elem(wv.z, gv.z, av.z, sc, lr_k, momentum, nesterov);
                   momentum_elem(wv.w, gv.w, av.w, sc, lr_k, momentum, nesterov);
                   vec4(a, v0, i) = av;
                   vec4(w, v0, i) = wv;
               });
}

__device__ __forceinline__ void momentum_apply_body(float* __restrict__ w, const float* __restrict__ g, float* __restrict__ a,
                                                    const tier_table& tt, float lr, float momentum, bool nesterov, float clip_norm,
                                                    const float* __restrict__ sumsq, float gscale, int64_t i0, int64_t step) {
    const float sc = clip_scale(clip_norm, sumsq, gscale);
    const int phase = align_phase(w, g, a, nullptr);
    for (int k = 0; k < tt.n; ++k)
        momentum_range(w, g, a, tt.t[k].begin, tt.t[k].end, phase, sc, lr * tt.t[k].lr_mult, momentum, nesterov, i0, step);
}

// One kernel per rule for the eager and the step-state (_st) entry points.  st != nullptr: lr / Adam's step size / the rate is read from
// the step state (vltf.h: vl_step_state), a uniform load, in place of the argument; nothing else differs, so a replayed update and the
// eager one get the same bits.  The state is read ahead of the skip word so that the two device loads are in flight together: read
// after it, the test of st cost every wave one more scalar round trip (+2 % on the Adam launch alone).
__global__ void momentum_apply_kernel(float* __restrict__ w, const float* __restrict__ g, float* __restrict__ a, tier_table tt, float lr,
                                      const vl_step_state* __restrict__ st, float momentum, int nesterov, float clip_norm,
                                      const float* __restrict__ sumsq, float gscale, const uint32_t* __restrict__ skip) {
    if (st) lr = st->lr;                                              // ahead of the skip word: the two loads share a round trip
    if (skip && *skip) return;
    momentum_apply_body(w, g, a, tt, lr, momentum, nesterov != 0, clip_norm, sumsq, gscale,
                        (int64_t)blockIdx.x * blockDim.x + threadIdx.x, (int64_t)gridDim.x * blockDim.x);
}

__global__ void sgd_apply_kernel(float* __restrict__ w, const float* __restrict__ g, tier_table tt, float lr,
                                 const vl_step_state* __restrict__ st, float clip_norm, const float* __restrict__ sumsq, float gscale,
                                 const uint32_t* __restrict__ skip) {
    if (st) lr = st->lr;
    if (skip && *skip) return;                                        // the step's results are invalid (vl_status_or): no update
    sgd_apply_body(w, g, tt, lr, clip_norm, sumsq, gscale, (int64_t)blockIdx.x * blockDim.x + threadIdx.x,
                   (int64_t)gridDim.x * blockDim.x);
}

__global__ void adam_apply_kernel(float* __restrict__ w, const float* __restrict__ g, float* __restrict__ m, float* __restrict__ v,
                                  tier_table tt, float lr_t, const vl_step_state* __restrict__ st, float clip_norm,
                                  const float* __restrict__ sumsq, float gscale, const uint32_t* __restrict__ skip) {
    if (st) lr_t = st->adam_lr;
    if (skip && *skip) return;
    adam_apply_body(w, g, m, v, tt, lr_t, clip_norm, sumsq, gscale, (int64_t)blockIdx.x * blockDim.x + threadIdx.x,
                    (int64_t)gridDim.x * blockDim.x);
}

// *dst |= first word of an LSTM cluster workspace (its sticky time-out word, lstm_cluster.hip): the optimizer's `skip` word of a step
__global__ void status_or_kernel(uint32_t* __restrict__ dst, const uint32_t* __restrict__ src, int init) {
    const uint32_t old = init ? 0u : *dst;
    *dst = (*src != 0u) ? 1u : old;
}
extern "C" int vl_status_or(uint32_t* dst, const void* lstm_ws, int init, vl_stream_t stream) {
    VL_CHECK(dst && lstm_ws, "vl_status_or: null argument");
    hipLaunchKernelGGL(status_or_kernel, dim3(1), dim3(1), 0, (hipStream_t)stream, dst, (const uint32_t*)lstm_ws, init);
    VL_LAUNCH_CHECK();
    return 0;
}

// state: nullptr (the eager entry points: lr / lr_t counts) or the step state the kernel reads in its place
static int sgd_apply_launch(float* w, const float* g, int64_t count, const tier_table& tt, float lr, const vl_step_state* state,
                            float clip_norm, const float* sumsq, float gscale, const uint32_t* skip, vl_stream_t stream) {
    hipLaunchKernelGGL(sgd_apply_kernel, dim3(grid_for(count, 256, 4096)), dim3(256), 0, (hipStream_t)stream, w, g, tt, lr, state,
                       clip_norm, sumsq, gscale, skip);
    VL_LAUNCH_CHECK();
    return 0;
}

extern "C" int vl_sgd_apply(float* w, const float* g, int64_t count, float lr, float clip_norm, const float* sumsq, float gscale,
                            const uint32_t* skip, vl_stream_t stream) {
    VL_CHECK(w && g && count > 0, "vl_sgd_apply: bad argument");
    return sgd_apply_launch(w, g, count, tier_table_full(count), lr, nullptr, clip_norm, sumsq, gscale, skip, stream);
}

extern "C" int vl_sgd_apply_tiers(float* w, const float* g, int64_t count, float lr, float clip_norm, const float* sumsq, float gscale,
                                  const uint32_t* skip, const vl_lr_tier* tiers, int n_tiers, vl_stream_t stream) {
    VL_CHECK(w && g && count > 0, "vl_sgd_apply_tiers: bad argument");
    tier_table tt;
    if (int rc = tier_table_make("vl_sgd_apply_tiers", tiers, n_tiers, count, &tt)) return rc;
    return sgd_apply_launch(w, g, count, tt, lr, nullptr, clip_norm, sumsq, gscale, skip, stream);
}

// Adam's bias-corrected step size at count `step` (TF: lr * sqrt(1 - beta2^t) / (1 - beta1^t)); host code, shared by vl_adam_apply and
// vl_step_state_set so that a replayed update and the eager one get the same bits
static float adam_step_size(float lr, int step) {
    const double b1t = 1.0 - pow(0.9, (double)step), b2t = 1.0 - pow(0.999, (double)step);
    return (float)(lr * sqrt(b2t) / b1t);
}

static int adam_apply_launch(float* w, const float* g, float* m, float* v, int64_t count, const tier_table& tt, float lr_t,
                             const vl_step_state* state, float clip_norm, const float* sumsq, float gscale, const uint32_t* skip,
                             vl_stream_t stream) {
    hipLaunchKernelGGL(adam_apply_kernel, dim3(grid_for(count, 256, 4096)), dim3(256), 0, (hipStream_t)stream, w, g, m, v, tt,
                       lr_t, state, clip_norm, sumsq, gscale, skip);
    VL_LAUNCH_CHECK();
    return 0;
}

extern "C" int vl_adam_apply(float* w, const float* g, float* m, float* v, int64_t count, float lr, float clip_norm,
                             const float* sumsq, float gscale, int step, const uint32_t* skip, vl_stream_t stream) {
    VL_CHECK(w && g && m && v && count > 0 && step >= 1, "vl_adam_apply: bad argument");
    return adam_apply_launch(w, g, m, v, count, tier_table_full(count), adam_step_size(lr, step), nullptr, clip_norm, sumsq, gscale, skip,
                             stream);
}

extern "C" int vl_adam_apply_tiers(float* w, const float* g, float* m, float* v, int64_t count, float lr, float clip_norm,
                                   const float* sumsq, float gscale, int step, const uint32_t* skip, const vl_lr_tier* tiers, int n_tiers,
                                   vl_stream_t stream) {
    VL_CHECK(w && g && m && v && count > 0 && step >= 1, "vl_adam_apply_tiers: bad argument");
    tier_table tt;
    if (int rc = tier_table_make("vl_adam_apply_tiers", tiers, n_tiers, count, &tt)) return rc;
    return adam_apply_launch(w, g, m, v, count, tt, adam_step_size(lr, step), nullptr, clip_norm, sumsq, gscale, skip, stream);
}

// ---- step state (vltf.h: vl_step_state): the scalars a replayed step reads from device memory -------------------------------
static_assert(sizeof(vl_step_state) == 32, "vl_step_state layout");

__global__ void step_state_set_kernel(vl_step_state* __restrict__ st, int64_t step, float lr, uint32_t tag_origin, float adam_lr) {
    st->step = step;
    st->lr = lr;
    st->tag_origin = tag_origin;
    st->adam_lr = adam_lr;
}

extern "C" size_t vl_step_state_bytes(void) { return sizeof(vl_step_state); }

// update_step: the count behind Adam's step size; draw_step: what state->step holds, the dropout seed's input.  They differ only under
// gradient accumulation, where the micro-steps of one update draw different masks.
static int step_state_write(const char* who, vl_step_state* state, int64_t update_step, int64_t draw_step, float lr, uint32_t tag_origin,
                            vl_stream_t stream) {
    VL_CHECK(state && update_step >= 0 && update_step < INT32_MAX && draw_step >= 0, "%s: bad argument", who);
    hipLaunchKernelGGL(step_state_set_kernel, dim3(1), dim3(1), 0, (hipStream_t)stream, state, draw_step, lr, tag_origin,
                       adam_step_size(lr, (int)update_step + 1));
    VL_LAUNCH_CHECK();
    return 0;
}

extern "C" int vl_step_state_set(vl_step_state* state, int64_t step, float lr, uint32_t tag_origin, vl_stream_t stream) {
    return step_state_write("vl_step_state_set", state, step, step, lr, tag_origin, stream);
}

extern "C" int vl_step_state_set_micro(vl_step_state* state, int64_t update_step, int64_t draw_step, float lr, uint32_t tag_origin,
                                       vl_stream_t stream) {
    return step_state_write("vl_step_state_set_micro", state, update_step, draw_step, lr, tag_origin, stream);
}

// the weight average's rate: a field of its own, written by a launch of its own (vl_step_state_set / _set_micro stay as they are)
static_assert(offsetof(vl_step_state, ema_rate) == 20, "vl_step_state layout");

__global__ void step_state_set_ema_kernel(vl_step_state* __restrict__ st, float rate) { st->ema_rate = rate; }

extern "C" int vl_step_state_set_ema(vl_step_state* state, float rate, vl_stream_t stream) {
    VL_CHECK(state, "vl_step_state_set_ema: bad argument");
    VL_CHECK(rate > 0.f && rate <= 1.f, "vl_step_state_set_ema: rate must lie in (0, 1], got %g", (double)rate);   // (NaN fails)
    hipLaunchKernelGGL(step_state_set_ema_kernel, dim3(1), dim3(1), 0, (hipStream_t)stream, state, rate);
    VL_LAUNCH_CHECK();
    return 0;
}

// the update entry points above with lr / Adam's step size read from the step state: the same kernels, handed the state
extern "C" int vl_sgd_apply_st(float* w, const float* g, int64_t count, const vl_step_state* state, float clip_norm, const float* sumsq,
                               float gscale, const uint32_t* skip, vl_stream_t stream) {
    VL_CHECK(w && g && state && count > 0, "vl_sgd_apply_st: bad argument");
    return sgd_apply_launch(w, g, count, tier_table_full(count), 0.f, state, clip_norm, sumsq, gscale, skip, stream);
}

extern "C" int vl_adam_apply_st(float* w, const float* g, float* m, float* v, int64_t count, const vl_step_state* state, float clip_norm,
                                const float* sumsq, float gscale, const uint32_t* skip, vl_stream_t stream) {
    VL_CHECK(w && g && m && v && state && count > 0, "vl_adam_apply_st: bad argument");
    return adam_apply_launch(w, g, m, v, count, tier_table_full(count), 0.f, state, clip_norm, sumsq, gscale, skip, stream);
}

extern "C" int vl_sgd_apply_tiers_st(float* w, const float* g, int64_t count, const vl_step_state* state, float clip_norm, const float* sumsq,
                                     float gscale, const uint32_t* skip, const vl_lr_tier* tiers, int n_tiers, vl_stream_t stream) {
    VL_CHECK(w && g && state && count > 0, "vl_sgd_apply_tiers_st: bad argument");
    tier_table tt;
    if (int rc = tier_table_make("vl_sgd_apply_tiers_st", tiers, n_tiers, count, &tt)) return rc;
    return sgd_apply_launch(w, g, count, tt, 0.f, state, clip_norm, sumsq, gscale, skip, stream);
}

extern "C" int vl_adam_apply_tiers_st(float* w, const float* g, float* m, float* v, int64_t count, const vl_step_state* state, float clip_norm,
                                      const float* sumsq, float gscale, const uint32_t* skip, const vl_lr_tier* tiers, int n_tiers,
                                      vl_stream_t stream) {
    VL_CHECK(w && g && m && v && state && count > 0, "vl_adam_apply_tiers_st: bad argument");
    tier_table tt;
    if (int rc = tier_table_make("vl_adam_apply_tiers_st", tiers, n_tiers, count, &tt)) return rc;
    return adam_apply_launch(w, g, m, v, count, tt, 0.f, state, clip_norm, sumsq, gscale, skip, stream);
}

// ---- momentum / Nesterov update (vltf.h: vl_momentum_apply): two entry points, a NULL table is the full range ---------------------
static int momentum_apply_launch(const char* who, float* w, const float* g, float* accum, int64_t count, float lr, const vl_step_state* state,
                                 float momentum, int nesterov, float clip_norm, const float* sumsq, float gscale, const uint32_t* skip,
                                 const vl_lr_tier* tiers, int n_tiers, vl_stream_t stream) {
    VL_CHECK(w && g && accum && count > 0, "%s: bad argument", who);
    VL_CHECK(momentum > 0.f && momentum < 1.f, "%s: momentum must lie in (0, 1), got %g", who, (double)momentum);   // (NaN fails)
    tier_table tt;
    if (int rc = tier_table_make(who, tiers, n_tiers, count, &tt, true)) return rc;
    hipLaunchKernelGGL(momentum_apply_kernel, dim3(grid_for(count, 256, 4096)), dim3(256), 0, (hipStream_t)stream, w, g, accum, tt, lr, state,
                       momentum, nesterov, clip_norm, sumsq, gscale, skip);
    VL_LAUNCH_CHECK();
    return 0;
}

extern "C" int vl_momentum_apply(float* w, const float* g, float* accum, int64_t count, float lr, float momentum, int nesterov,
                                 float clip_norm, const float* sumsq, float gscale, const uint32_t* skip, const vl_lr_tier* tiers,
                                 int n_tiers, vl_stream_t stream) {
    return momentum_apply_launch("vl_momentum_apply", w, g, accum, count, lr, nullptr, momentum, nesterov, clip_norm, sumsq, gscale, skip,
                                 tiers, n_tiers, stream);
}

extern "C" int vl_momentum_apply_st(float* w, const float* g, float* accum, int64_t count, const vl_step_state* state, float momentum,
                                    int nesterov, float clip_norm, const float* sumsq, float gscale, const uint32_t* skip,
                                    const vl_lr_tier* tiers, int n_tiers, vl_stream_t stream) {
    VL_CHECK(state, "vl_momentum_apply_st: bad argument");
    return momentum_apply_launch("vl_momentum_apply_st", w, g, accum, count, 0.f, state, momentum, nesterov, clip_norm, sumsq, gscale, skip,
                                 tiers, n_tiers, stream);
}

// ---- gradient accumulation over micro-batches (vltf.h: vl_grad_accumulate) ------------------------------------------------------------
// MODE 0: acc = g.  MODE 1: acc = acc + g.  MODE 2: g = acc + g (acc stays).  One fp32 add per element, shared by the scalar head / tail
// and the 16-byte interior; the ranges go through range_walk, so an element outside every range is never addressed.
__device__ __forceinline__ float acc_elem(float a, float g) {
#pragma clang fp contract(off)
    return a + g;
}

template <int MODE>
__global__ __launch_bounds__(256) void grad_accumulate_kernel(float* __restrict__ acc, float* __restrict__ g, tier_table tt) {
    const int64_t i0 = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, step = (int64_t)gridDim.x * blockDim.x;
    const int phase = align_phase(acc, g, nullptr, nullptr);
    for (int k = 0; k < tt.n; ++k)
        range_walk(tt.t[k].begin, tt.t[k].end, phase, i0, step,
                   [&](int64_t i) {
                       if (MODE == 0) acc[i] = g[i];
                       else if (MODE == 1) acc[i] = acc_elem(acc[i], g[i]);
                       else g[i] = acc_elem(acc[i], g[i]);
                   },
                   [&](int64_t v0, int64_t i) {
                       const float4 gv = vec4(g, v0, i);
                       if (MODE == 0) {
                           vec4(acc, v0, i) = gv;
                       } else {
                           const float4 av = vec4(acc, v0, i);
                           float4 r;
                           r.x = acc_elem(av.x, gv.x);
                           r.y = acc_elem(av.y, gv.y);
                           r.z = acc_elem(av.z, gv.z);
                           r.w = acc_elem(av.w, gv.w);
                           if (MODE == 1) vec4(acc, v0, i) = r;
                           else vec4(g, v0, i) = r;
                       }
                   });
}

extern "C" int vl_grad_accumulate(float* acc, float* g, int64_t count, int mode, const vl_lr_tier* ranges, int n_ranges,
                                  vl_stream_t stream) {
    VL_CHECK(acc && g && count > 0, "vl_grad_accumulate: bad argument");
    VL_CHECK(mode >= 0 && mode <= 2, "vl_grad_accumulate: mode must be 0 (store), 1 (add) or 2 (final), got %d", mode);
    tier_table tt;
    if (int rc = tier_table_make("vl_grad_accumulate", ranges, n_ranges, count, &tt, true)) return rc;
    const dim3 grid(grid_for(count, 256, 4096)), block(256);
    if (mode == 0) hipLaunchKernelGGL(grad_accumulate_kernel<0>, grid, block, 0, (hipStream_t)stream, acc, g, tt);
    else if (mode == 1) hipLaunchKernelGGL(grad_accumulate_kernel<1>, grid, block, 0, (hipStream_t)stream, acc, g, tt);
    else hipLaunchKernelGGL(grad_accumulate_kernel<2>, grid, block, 0, (hipStream_t)stream, acc, g, tt);
    VL_LAUNCH_CHECK();
    return 0;
}

// ---- exponential moving average of the weights (vltf.h: vl_ema_update) ------------------------------------------------------------------
// s' = fma(rate, w - s, s): two roundings, spelled out, shared by the scalar head / tail and the 16-byte interior; the ranges are walked
// by range_walk, so an element outside every range is never addressed.
__device__ __forceinline__ float ema_elem(float s, float w, float rate) {
#pragma clang fp contract(off)
    const float d = w - s;
    return __builtin_fmaf(rate, d, s);
}

__device__ __forceinline__ void ema_update_body(float* __restrict__ s, const float* __restrict__ w, const tier_table& tt, float rate, int64_t i0,
                                                int64_t step) {
    const int phase = align_phase(s, w, nullptr, nullptr);
    for (int k = 0; k < tt.n; ++k)
        range_walk(tt.t[k].begin, tt.t[k].end, phase, i0, step, [&](int64_t i) { s[i] = ema_elem(s[i], w[i], rate); },
                   [&](int64_t v0, int64_t i) {
                       float4 sv = vec4(s, v0, i);
                       const float4 wv = vec4(w, v0, i);
                       sv.x = ema_elem(sv.x, wv.x, rate);
                       sv.y = ema_elem(sv.y, wv.y, rate);
                       sv.z = ema_elem(sv.z, wv.z, rate);
                       sv.w = ema_elem(sv.w, wv.w, rate);
                       vec4(s, v0, i) = sv;
                   });
}

// st != nullptr: the rate from the state (momentum_apply_kernel)
__global__ void ema_update_kernel(float* __restrict__ s, const float* __restrict__ w, tier_table tt, float rate,
                                  const vl_step_state* __restrict__ st, const uint32_t* __restrict__ skip) {
    if (st) rate = st->ema_rate;
    if (skip && *skip) return;
    ema_update_body(s, w, tt, rate, (int64_t)blockIdx.x * blockDim.x + threadIdx.x, (int64_t)gridDim.x * blockDim.x);
}

// state == nullptr: the rate counts, and is checked
static int ema_update_launch(const char* who, float* shadow, const float* w, int64_t count, float rate, const vl_step_state* state,
                             const uint32_t* skip, const vl_lr_tier* ranges, int n_ranges, vl_stream_t stream) {
    VL_CHECK(shadow && w && count > 0, "%s: bad argument", who);
    tier_table tt;
    if (int rc = tier_table_make(who, ranges, n_ranges, count, &tt, true)) return rc;
    VL_CHECK(state || (rate > 0.f && rate <= 1.f), "%s: rate must lie in (0, 1], got %g", who, (double)rate);   // (NaN fails)
    hipLaunchKernelGGL(ema_update_kernel, dim3(grid_for(count, 256, 4096)), dim3(256), 0, (hipStream_t)stream, shadow, w, tt, rate, state,
                       skip);
    VL_LAUNCH_CHECK();
    return 0;
}

extern "C" int vl_ema_update(float* shadow, const float* w, int64_t count, float rate, const uint32_t* skip, const vl_lr_tier* ranges,
                             int n_ranges, vl_stream_t stream) {
    return ema_update_launch("vl_ema_update", shadow, w, count, rate, nullptr, skip, ranges, n_ranges, stream);
}

extern "C" int vl_ema_update_st(float* shadow, const float* w, int64_t count, const vl_step_state* state, const uint32_t* skip,
                                const vl_lr_tier* ranges, int n_ranges, vl_stream_t stream) {
    VL_CHECK(state, "vl_ema_update_st: bad argument");
    return ema_update_launch("vl_ema_update_st", shadow, w, count, 0.f, state, skip, ranges, n_ranges, stream);
}

// ---- per-variable gradient / weight statistics (vltf.h: vl_tensor_stats) ----------------------------------------------------------------
// A segmented two-stage reduction in fp64.  The order is a property of the table alone: element j of a chunk goes, in order of j, into
// accumulator j mod 1024 of its chunk ("slot"), the slots are summed in a fixed tree, the chunk rows of a segment likewise.  A thread
// reads the 16-byte vectors v = t, t + 256, ... of its chunk counted from the aligned address at or before the chunk's first element,
// r = 0 .. 3 elements earlier: component c of vector v is element j = 4 v + c - r, so (thread, component) always feeds slot
// (4 t + c - r) mod 1024 and where the vectors begin changes only WHO holds a slot, never what is added to it or in which order.
constexpr int STAT_SLOTS = 1024;
static_assert(sizeof(vl_tensor_stat) == 64, "vl_tensor_stat is 64 bytes");
static_assert((VL_STAT_CHUNK & (VL_STAT_CHUNK - 1)) == 0 && VL_STAT_CHUNK % STAT_SLOTS == 0, "VL_STAT_CHUNK: a power of two, whole slot rounds");

struct stat_table {
    vl_stat_segment seg[VL_MAX_STAT_SEGMENTS];
    int first[VL_MAX_STAT_SEGMENTS + 1];      // a segment's first chunk index; first[n] = the chunks of the whole table
    int n;
};

// count < 0: the bound of the buffers is not known (vl_tensor_stats_ws_bytes)
static int stat_table_make(const char* who, const vl_stat_segment* segs, int n_segs, int64_t count, stat_table* out) {
    VL_CHECK(segs && n_segs >= 1 && n_segs <= VL_MAX_STAT_SEGMENTS, "%s: 1 .. %d segments, got %d", who, VL_MAX_STAT_SEGMENTS, n_segs);
    int64_t prev = 0;
    int chunks = 0;
    for (int k = 0; k < n_segs; ++k) {
        const vl_stat_segment& s = segs[k];
        VL_CHECK(s.begin >= prev && s.end > s.begin && (count < 0 || s.end <= count),
                 "%s: segment %d = [%lld, %lld) is empty, unsorted, overlaps its predecessor or leaves [0, %lld)", who, k, (long long)s.begin,
                 (long long)s.end, (long long)count);
        VL_CHECK(s.end - s.begin <= 0xFFFFFFFFll, "%s: segment %d has %lld elements, more than 2^32 - 1", who, k, (long long)(s.end - s.begin));
        out->seg[k] = s;
        out->first[k] = chunks;
        chunks += (int)((s.end - s.begin + VL_STAT_CHUNK - 1) / VL_STAT_CHUNK);
        prev = s.end;
    }
    out->first[n_segs] = chunks;
    out->n = n_segs;
    return 0;
}

// floats as ints of the same order, -0 below +0: min / max of the keys are exact and do not depend on the order of the operands
constexpr int STAT_KEY_PINF = 0x7f800000, STAT_KEY_NINF = (int)0x807fffffu;
__device__ __forceinline__ int stat_key(float x) {
    const int k = __float_as_int(x);
    return k ^ ((k >> 31) & 0x7fffffff);
}
__device__ __forceinline__ float stat_unkey(int k) { return __int_as_float(k ^ ((k >> 31) & 0x7fffffff)); }

struct stat_acc {
    double d[4];              // g_sum, g_sumsq, w_sum, w_sumsq
    int mn[2], mx[2];         // keys of g / w min and max
    uint32_t cnt[3];          // g_nonfinite, w_nonfinite, g_zero
};
__device__ __forceinline__ void stat_acc_init(stat_acc& a) {
    a.d[0] = a.d[1] = a.d[2] = a.d[3] = 0.0;
    a.mn[0] = a.mn[1] = STAT_KEY_PINF;
    a.mx[0] = a.mx[1] = STAT_KEY_NINF;
    a.cnt[0] = a.cnt[1] = a.cnt[2] = 0u;
}

// one element function for the 4-byte and the 16-byte loads.  Finite, zero and the order keys are read off the bits, so no denormal mode
// plays a part; a non-finite element adds +0 to the sums and the neutral key to min / max.
__device__ __forceinline__ void stat_elem(float w, float g, double& gs, double& gq, double& wsum, double& wq, stat_acc& a) {
    const int gb = __float_as_int(g), wb = __float_as_int(w);
    const bool gf = (gb & 0x7f800000) != 0x7f800000, wf = (wb & 0x7f800000) != 0x7f800000;
    const double gd = gf ? (double)g : 0.0, wd = wf ? (double)w : 0.0;
    gs += gd;
    gq = __builtin_fma(gd, gd, gq);           // the product of two fp32 values is exact in fp64: one rounding, that of the sum
    wsum += wd;
    wq = __builtin_fma(wd, wd, wq);
    const int gk = stat_key(g), wk = stat_key(w);
    a.mn[0] = min(a.mn[0], gf ? gk : STAT_KEY_PINF);
    a.mx[0] = max(a.mx[0], gf ? gk : STAT_KEY_NINF);
    a.mn[1] = min(a.mn[1], wf ? wk : STAT_KEY_PINF);
    a.mx[1] = max(a.mx[1], wf ? wk : STAT_KEY_NINF);
    a.cnt[0] += gf ? 0u : 1u;
    a.cnt[1] += wf ? 0u : 1u;
    a.cnt[2] += (gb & 0x7fffffff) == 0 ? 1u : 0u;
}

// every lane of the block ends with the block's totals: xor butterfly inside a wave, then the four waves in wave order
__device__ __forceinline__ void stat_block_reduce(stat_acc& a, double* smd /* [16] */, int* smi /* [28] */) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
#pragma unroll
        for (int q = 0; q < 4; ++q) a.d[q] += __shfl_xor(a.d[q], o, 64);
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            a.mn[q] = min(a.mn[q], __shfl_xor(a.mn[q], o, 64));
            a.mx[q] = max(a.mx[q], __shfl_xor(a.mx[q], o, 64));
        }
#pragma unroll
        for (int q = 0; q < 3; ++q) a.cnt[q] += (uint32_t)__shfl_xor((int)a.cnt[q], o, 64);
    }
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    if (lane == 0) {
        for (int q = 0; q < 4; ++q) smd[wv * 4 + q] = a.d[q];
        for (int q = 0; q < 2; ++q) {
            smi[wv * 7 + q] = a.mn[q];
            smi[wv * 7 + 2 + q] = a.mx[q];
        }
        for (int q = 0; q < 3; ++q) smi[wv * 7 + 4 + q] = (int)a.cnt[q];
    }
    __syncthreads();
    for (int q = 0; q < 4; ++q) a.d[q] = ((smd[q] + smd[4 + q]) + smd[8 + q]) + smd[12 + q];
    for (int q = 0; q < 2; ++q) {
        a.mn[q] = min(min(smi[q], smi[7 + q]), min(smi[14 + q], smi[21 + q]));
        a.mx[q] = max(max(smi[2 + q], smi[9 + q]), max(smi[16 + q], smi[23 + q]));
    }
    for (int q = 0; q < 3; ++q) a.cnt[q] = (uint32_t)smi[4 + q] + (uint32_t)smi[11 + q] + (uint32_t)smi[18 + q] + (uint32_t)smi[25 + q];
    __syncthreads();
}

__device__ __forceinline__ void stat_row_store(vl_tensor_stat* row, const stat_acc& a) {
    vl_tensor_stat r;
    r.g_sum = a.d[0];
    r.g_sumsq = a.d[1];
    r.w_sum = a.d[2];
    r.w_sumsq = a.d[3];
    r.g_min = stat_unkey(a.mn[0]);
    r.g_max = stat_unkey(a.mx[0]);
    r.w_min = stat_unkey(a.mn[1]);
    r.w_max = stat_unkey(a.mx[1]);
    r.g_nonfinite = a.cnt[0];
    r.w_nonfinite = a.cnt[1];
    r.g_zero = a.cnt[2];
    r.reserved = 0u;
    *row = r;
}

// one workgroup per chunk -> ws[chunk]
__global__ __launch_bounds__(256) void tensor_stats_stage1(const float* __restrict__ w, const float* __restrict__ g, stat_table st,
                                                           vl_tensor_stat* __restrict__ ws) {
    __shared__ double sl[4][STAT_SLOTS];
    const int b = blockIdx.x, t = threadIdx.x;
    int s = 0;
    for (int k = 1; k < st.n; ++k)
        if (st.first[k] <= b) s = k;
    const int64_t cb = st.seg[s].begin + (int64_t)(b - st.first[s]) * VL_STAT_CHUNK;
    const int64_t rest = st.seg[s].end - cb;
    const int len = rest < VL_STAT_CHUNK ? (int)rest : VL_STAT_CHUNK;
    const int phase = align_phase(w, g, nullptr, nullptr);
    const int r = phase < 0 ? 0 : (int)((cb + phase) & 3);
    const int64_t base = cb - r;              // the element of vector 0, component 0: 16-byte aligned in w and in g when phase >= 0
    const int nv = (len + r + 3) >> 2;
    double gs[4] = {0.0, 0.0, 0.0, 0.0}, gq[4] = {0.0, 0.0, 0.0, 0.0}, wsum[4] = {0.0, 0.0, 0.0, 0.0}, wq[4] = {0.0, 0.0, 0.0, 0.0};
    stat_acc a;
    stat_acc_init(a);
    constexpr int U = 4;
    for (int v0 = t; v0 < nv; v0 += 256 * U) {
        if (phase >= 0 && 4 * v0 >= r && 4 * (v0 + 256 * (U - 1)) + 4 - r <= len) {      // U whole vectors: every load issued first
            float4 wv[U], gv[U];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                wv[u] = *reinterpret_cast<const float4*>(w + base + 4 * (int64_t)(v0 + 256 * u));
                gv[u] = *reinterpret_cast<const float4*>(g + base + 4 * (int64_t)(v0 + 256 * u));
            }
#pragma unroll
            for (int u = 0; u < U; ++u) {
                stat_elem(wv[u].x, gv[u].x, gs[0], gq[0], wsum[0], wq[0], a);
                stat_elem(wv[u].y, gv[u].y, gs[1], gq[1], wsum[1], wq[1], a);
                stat_elem(wv[u].z, gv[u].z, gs[2], gq[2], wsum[2], wq[2], a);
                stat_elem(wv[u].w, gv[u].w, gs[3], gq[3], wsum[3], wq[3], a);
            }
            continue;
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int v = v0 + 256 * u;
            if (v >= nv) break;
            const int j0 = 4 * v - r;         // the chunk index of component 0
            const int64_t e = base + 4 * (int64_t)v;
            if (phase >= 0 && j0 >= 0 && j0 + 4 <= len) {
                const float4 wv = *reinterpret_cast<const float4*>(w + e), gv = *reinterpret_cast<const float4*>(g + e);
                stat_elem(wv.x, gv.x, gs[0], gq[0], wsum[0], wq[0], a);
                stat_elem(wv.y, gv.y, gs[1], gq[1], wsum[1], wq[1], a);
                stat_elem(wv.z, gv.z, gs[2], gq[2], wsum[2], wq[2], a);
                stat_elem(wv.w, gv.w, gs[3], gq[3], wsum[3], wq[3], a);
            } else {                          // the chunk's head or tail, or w and g disagree in phase: only elements of the chunk are addressed
#pragma unroll
                for (int c = 0; c < 4; ++c)
                    if (j0 + c >= 0 && j0 + c < len) stat_elem(w[e + c], g[e + c], gs[c], gq[c], wsum[c], wq[c], a);
            }
        }
    }
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        const int slot = (4 * t + c - r) & (STAT_SLOTS - 1);
        sl[0][slot] = gs[c];
        sl[1][slot] = gq[c];
        sl[2][slot] = wsum[c];
        sl[3][slot] = wq[c];
    }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < 4; ++q) a.d[q] = ((sl[q][4 * t] + sl[q][4 * t + 1]) + sl[q][4 * t + 2]) + sl[q][4 * t + 3];
    __syncthreads();
    stat_block_reduce(a, &sl[0][0], reinterpret_cast<int*>(&sl[1][0]));
    if (t == 0) stat_row_store(ws + b, a);
}

// one workgroup per segment: its chunk rows in the order row t, t + 256, ... per thread, then the block's tree -> out[segment]
__global__ __launch_bounds__(256) void tensor_stats_stage2(const vl_tensor_stat* __restrict__ ws, stat_table st,
                                                           vl_tensor_stat* __restrict__ out) {
    __shared__ double smd[16];
    __shared__ int smi[28];
    const int s = blockIdx.x;
    stat_acc a;
    stat_acc_init(a);
    for (int i = st.first[s] + (int)threadIdx.x; i < st.first[s + 1]; i += 256) {
        const vl_tensor_stat r = ws[i];
        a.d[0] += r.g_sum;
        a.d[1] += r.g_sumsq;
        a.d[2] += r.w_sum;
        a.d[3] += r.w_sumsq;
        a.mn[0] = min(a.mn[0], stat_key(r.g_min));
        a.mx[0] = max(a.mx[0], stat_key(r.g_max));
        a.mn[1] = min(a.mn[1], stat_key(r.w_min));
        a.mx[1] = max(a.mx[1], stat_key(r.w_max));
        a.cnt[0] += r.g_nonfinite;
        a.cnt[1] += r.w_nonfinite;
        a.cnt[2] += r.g_zero;
    }
    stat_block_reduce(a, smd, smi);
    if (threadIdx.x == 0) stat_row_store(out + s, a);
}

extern "C" size_t vl_tensor_stats_ws_bytes(const vl_stat_segment* segs, int n_segs) {
    stat_table st;
    if (stat_table_make("vl_tensor_stats_ws_bytes", segs, n_segs, -1, &st)) return 0;
    return (size_t)st.first[st.n] * sizeof(vl_tensor_stat);
}

extern "C" int vl_tensor_stats(const float* w, const float* g, int64_t count, const vl_stat_segment* segs, int n_segs, vl_tensor_stat* out,
                               void* ws, size_t ws_bytes, vl_stream_t stream) {
    VL_CHECK(w && g && out && ws && count > 0, "vl_tensor_stats: bad argument");
    VL_CHECK((((uintptr_t)w | (uintptr_t)g) & 3) == 0 && (((uintptr_t)out | (uintptr_t)ws) & 7) == 0, "vl_tensor_stats: misaligned pointer");
    stat_table st;
    if (int rc = stat_table_make("vl_tensor_stats", segs, n_segs, count, &st)) return rc;
    const size_t need = (size_t)st.first[st.n] * sizeof(vl_tensor_stat);
    VL_CHECK(ws_bytes >= need, "vl_tensor_stats: the workspace has %zu bytes, this table needs %zu (vl_tensor_stats_ws_bytes)", ws_bytes, need);
    hipLaunchKernelGGL(tensor_stats_stage1, dim3(st.first[st.n]), dim3(256), 0, (hipStream_t)stream, w, g, st,
                       reinterpret_cast<vl_tensor_stat*>(ws));
    VL_LAUNCH_CHECK();
    hipLaunchKernelGGL(tensor_stats_stage2, dim3(st.n), dim3(256), 0, (hipStream_t)stream, reinterpret_cast<const vl_tensor_stat*>(ws), st, out);
    VL_LAUNCH_CHECK();
    return 0;
}

// ---- LARS (vltf.h: vl_lars_trust, vl_lars_apply): a per-variable trust ratio on the device, then the momentum update through it ----------
struct lars_decay {
    float d[VL_MAX_STAT_SEGMENTS];
};

// one workgroup, lane k = segment k: the row's two fp64 sums -> trust[k], in double, rounded to float once
__global__ __launch_bounds__(VL_MAX_STAT_SEGMENTS) void lars_trust_kernel(const vl_tensor_stat* __restrict__ rows, int n, double eeta,
                                                                          double eps, lars_decay dec, float clip_norm,
                                                                          const float* __restrict__ sumsq, float gscale,
                                                                          float* __restrict__ trust) {
#pragma clang fp contract(off)
    const int k = threadIdx.x;
    if (k >= n) return;
    const double sc = (double)clip_scale(clip_norm, sumsq, gscale);
    const double wn = sqrt(rows[k].w_sumsq), gn = sc * sqrt(rows[k].g_sumsq);
    const bool finite = rows[k].g_nonfinite == 0u && rows[k].w_nonfinite == 0u;
    float t = 1.f;
    if (finite && wn > 0.0 && gn > 0.0) t = (float)(eeta * wn / (gn + (double)dec.d[k] * wn + eps));      // (a NaN norm fails > 0)
    trust[k] = t;
}

extern "C" int vl_lars_trust(const vl_tensor_stat* rows, int n_segs, double eeta, double eps, const float* decay, float clip_norm,
                             const float* sumsq, float gscale, float* trust, vl_stream_t stream) {
    VL_CHECK(rows && decay && trust, "vl_lars_trust: bad argument");
    VL_CHECK(n_segs >= 1 && n_segs <= VL_MAX_STAT_SEGMENTS, "vl_lars_trust: 1 .. %d segments, got %d", VL_MAX_STAT_SEGMENTS, n_segs);
    VL_CHECK(((uintptr_t)rows & 7) == 0 && ((uintptr_t)trust & 3) == 0, "vl_lars_trust: misaligned pointer");
    VL_CHECK(eeta > 0.0 && eeta <= 1.7976931348623157e308, "vl_lars_trust: eeta must be finite and > 0, got %g", eeta);       // (NaN fails)
    VL_CHECK(eps >= 0.0 && eps <= 1.7976931348623157e308, "vl_lars_trust: eps must be finite and >= 0, got %g", eps);
    lars_decay dec;
    for (int k = 0; k < n_segs; ++k) {
        VL_CHECK(decay[k] >= 0.f && decay[k] <= 3.402823466e38f, "vl_lars_trust: segment %d: decay must be finite and >= 0", k);
        dec.d[k] = decay[k];
    }
    for (int k = n_segs; k < VL_MAX_STAT_SEGMENTS; ++k) dec.d[k] = 0.f;
    hipLaunchKernelGGL(lars_trust_kernel, dim3(1), dim3(VL_MAX_STAT_SEGMENTS), 0, (hipStream_t)stream, rows, n_segs, eeta, eps, dec, clip_norm,
                       sumsq, gscale, trust);
    VL_LAUNCH_CHECK();
    return 0;
}

struct lars_table {
    vl_lars_range r[VL_MAX_STAT_SEGMENTS];
    int n;
};

// the rules of tier_table_make, and every trust_index is -1 or inside the trust array (the kernel reads trust[index] unchecked)
static int lars_table_make(const char* who, const vl_lars_range* ranges, int n_ranges, int64_t count, const float* trust, int n_trust,
                           lars_table* out) {
    VL_CHECK(ranges && n_ranges >= 1 && n_ranges <= VL_MAX_STAT_SEGMENTS, "%s: 1 .. %d ranges, got %d", who, VL_MAX_STAT_SEGMENTS, n_ranges);
    VL_CHECK(n_trust >= 0 && (trust || n_trust == 0), "%s: a trust array of %d entries at a null pointer", who, n_trust);
    int64_t prev = 0;
    for (int k = 0; k < n_ranges; ++k) {
        const vl_lars_range& r = ranges[k];
        if (int rc = range_bounds_check(who, "range ", k, "", r.begin, r.end, prev, count)) return rc;
        if (int rc = range_factor_check(who, "range ", k, "", "lr_mult", r.lr_mult, true)) return rc;
        VL_CHECK(r.trust_index >= -1 && r.trust_index < n_trust, "%s: range %d: trust_index %d is neither -1 nor inside the %d trust entries",
                 who, k, r.trust_index, n_trust);
        out->r[k] = r;
        prev = r.end;
    }
    out->n = n_ranges;
    return 0;
}

// momentum_apply_body with lr_k = (lr * lr_mult) * trust: the trust value is one uniform load per range, the elements are momentum_range's
__device__ __forceinline__ void lars_apply_body(float* __restrict__ w, const float* __restrict__ g, float* __restrict__ a, const lars_table& lt,
                                                const float* __restrict__ trust, float lr, float momentum, bool nesterov, float clip_norm,
                                                const float* __restrict__ sumsq, float gscale, int64_t i0, int64_t step) {
    const float sc = clip_scale(clip_norm, sumsq, gscale);
    const int phase = align_phase(w, g, a, nullptr);
    for (int k = 0; k < lt.n; ++k) {
        const int ti = lt.r[k].trust_index;
        const float lr_k = (lr * lt.r[k].lr_mult) * (ti < 0 ? 1.f : trust[ti]);
        momentum_range(w, g, a, lt.r[k].begin, lt.r[k].end, phase, sc, lr_k, momentum, nesterov, i0, step);
    }
}

// st != nullptr: lr from the state (momentum_apply_kernel)
__global__ void lars_apply_kernel(float* __restrict__ w, const float* __restrict__ g, float* __restrict__ a, lars_table lt,
                                  const float* __restrict__ trust, float lr, const vl_step_state* __restrict__ st, float momentum,
                                  int nesterov, float clip_norm, const float* __restrict__ sumsq, float gscale,
                                  const uint32_t* __restrict__ skip) {
    if (st) lr = st->lr;
    if (skip && *skip) return;
    lars_apply_body(w, g, a, lt, trust, lr, momentum, nesterov != 0, clip_norm, sumsq, gscale,
                    (int64_t)blockIdx.x * blockDim.x + threadIdx.x, (int64_t)gridDim.x * blockDim.x);
}

static int lars_apply_launch(const char* who, float* w, const float* g, float* accum, int64_t count, float lr, const vl_step_state* state,
                             float momentum, int nesterov, float clip_norm, const float* sumsq, float gscale, const uint32_t* skip,
                             const vl_lars_range* ranges, int n_ranges, const float* trust, int n_trust, vl_stream_t stream) {
    VL_CHECK(w && g && accum && count > 0, "%s: bad argument", who);
    VL_CHECK(momentum > 0.f && momentum < 1.f, "%s: momentum must lie in (0, 1), got %g", who, (double)momentum);   // (NaN fails)
    lars_table lt;
    if (int rc = lars_table_make(who, ranges, n_ranges, count, trust, n_trust, &lt)) return rc;
    hipLaunchKernelGGL(lars_apply_kernel, dim3(grid_for(count, 256, 4096)), dim3(256), 0, (hipStream_t)stream, w, g, accum, lt, trust, lr,
                       state, momentum, nesterov, clip_norm, sumsq, gscale, skip);
    VL_LAUNCH_CHECK();
    return 0;
}

extern "C" int vl_lars_apply(float* w, const float* g, float* accum, int64_t count, float lr, float momentum, int nesterov, float clip_norm,
                             const float* sumsq, float gscale, const uint32_t* skip, const vl_lars_range* ranges, int n_ranges,
                             const float* trust, int n_trust, vl_stream_t stream) {
    return lars_apply_launch("vl_lars_apply", w, g, accum, count, lr, nullptr, momentum, nesterov, clip_norm, sumsq, gscale, skip, ranges,
                             n_ranges, trust, n_trust, stream);
}

extern "C" int vl_lars_apply_st(float* w, const float* g, float* accum, int64_t count, const vl_step_state* state, float momentum,
                                int nesterov, float clip_norm, const float* sumsq, float gscale, const uint32_t* skip,
                                const vl_lars_range* ranges, int n_ranges, const float* trust, int n_trust, vl_stream_t stream) {
    VL_CHECK(state, "vl_lars_apply_st: bad argument");
    return lars_apply_launch("vl_lars_apply_st", w, g, accum, count, 0.f, state, momentum, nesterov, clip_norm, sumsq, gscale, skip, ranges,
                             n_ranges, trust, n_trust, stream);
}

// ---- LAMB (vltf.h: vl_lamb_moments, vl_lamb_apply): Adam's moments, a per-tensor trust ratio |w| / |u| on the device, decoupled decay -----
static_assert(sizeof(vl_lamb_range) == 32 && sizeof(vl_lamb_row) == 24, "vl_lamb_range / vl_lamb_row layout");
static_assert(offsetof(vl_step_state, reserved) == 24, "vl_step_state layout");

struct lamb_table {
    vl_lamb_range r[VL_MAX_STAT_SEGMENTS];
    int first[VL_MAX_STAT_SEGMENTS + 1];      // a range's first chunk index (stat_table's plan over ALL ranges); first[n] = the chunks of the table
    int n;
};

// the rules of lars_table_make plus a decay per range; count < 0: the bound of the buffers is not known (vl_lamb_moments_ws_bytes)
static int lamb_table_make(const char* who, const vl_lamb_range* ranges, int n_ranges, int64_t count, int n_trust, lamb_table* out) {
    VL_CHECK(ranges && n_ranges >= 1 && n_ranges <= VL_MAX_STAT_SEGMENTS, "%s: ranges: 1 .. %d entries, got %d", who, VL_MAX_STAT_SEGMENTS,
             n_ranges);
    int64_t prev = 0, chunks = 0;
    for (int k = 0; k < n_ranges; ++k) {
        const vl_lamb_range& r = ranges[k];
        if (int rc = range_bounds_check(who, "ranges[", k, "]", r.begin, r.end, prev, count)) return rc;
        VL_CHECK(r.end - r.begin <= 0x7FFFFFFFll, "%s: ranges[%d] has %lld elements, more than 2^31 - 1", who, k, (long long)(r.end - r.begin));
        if (int rc = range_factor_check(who, "ranges[", k, "]", "lr_mult", r.lr_mult, true)) return rc;
        if (int rc = range_factor_check(who, "ranges[", k, "]", "decay", r.decay, false)) return rc;
        VL_CHECK(r.trust_index >= -1 && (count < 0 || r.trust_index < n_trust),
                 "%s: ranges[%d]: trust_index %d is neither -1 nor inside the %d entries of trust", who, k, r.trust_index, n_trust);
        out->r[k] = r;
        out->first[k] = (int)chunks;
        chunks += (r.end - r.begin + VL_STAT_CHUNK - 1) / VL_STAT_CHUNK;
        VL_CHECK(chunks <= 0x7FFFFFFFll, "%s: ranges: more than 2^31 - 1 chunks", who);
        prev = r.end;
    }
    out->first[n_ranges] = (int)chunks;
    out->n = n_ranges;
    return 0;
}

// u of one element from the moments of THIS update: the one function vl_lamb_moments sums and vl_lamb_apply subtracts
__device__ __forceinline__ float lamb_dir(float w, float mi, float vi, float c1, float c2, float eps, float decay) {
#pragma clang fp contract(off)
    const float mh = mi * c1;
    const float vh = vi * c2;
    const float r = mh / (sqrtf(vh) + eps);
    return decay > 0.f ? __builtin_fmaf(decay, w, r) : r;
}

// adam_elem's two moment lines, unchanged
__device__ __forceinline__ void lamb_moment_elem(float g, float& m, float& v, float sc) {
#pragma clang fp contract(off)
    const float gi = g * sc;
    const float mi = __builtin_fmaf(0.9f, m, 0.1f * gi);
    const float vi = __builtin_fmaf(0.999f, v, gi * (0.001f * gi));
    m = mi;
    v = vi;
}

// stat_elem's w_sumsq lines for w and for u
__device__ __forceinline__ void lamb_stat_elem(float w, float u, double& wq, double& uq, uint32_t& bad) {
    const bool wf = (__float_as_int(w) & 0x7f800000) != 0x7f800000, uf = (__float_as_int(u) & 0x7f800000) != 0x7f800000;
    const double wd = wf ? (double)w : 0.0, ud = uf ? (double)u : 0.0;
    wq = __builtin_fma(wd, wd, wq);
    uq = __builtin_fma(ud, ud, uq);
    bad += (wf ? 0u : 1u) + (uf ? 0u : 1u);
}

struct lamb_consts {
    float sc, c1, c2, eps, decay;
};

template <bool NORMS>
__device__ __forceinline__ void lamb_moments_elem(float w, float g, float& m, float& v, const lamb_consts& k, double& wq, double& uq,
                                                  uint32_t& bad) {
    lamb_moment_elem(g, m, v, k.sc);
    if (NORMS) lamb_stat_elem(w, lamb_dir(w, m, v, k.c1, k.c2, k.eps, k.decay), wq, uq, bad);
}

// stat_block_reduce for two sums and one count: the same butterfly, the same wave order
__device__ __forceinline__ void lamb_block_reduce(double& wq, double& uq, uint32_t& bad, double* smd /* [8] */, uint32_t* smi /* [4] */) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        wq += __shfl_xor(wq, o, 64);
        uq += __shfl_xor(uq, o, 64);
        bad += (uint32_t)__shfl_xor((int)bad, o, 64);
    }
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    if (lane == 0) {
        smd[wv * 2] = wq;
        smd[wv * 2 + 1] = uq;
        smi[wv] = bad;
    }
    __syncthreads();
    wq = ((smd[0] + smd[2]) + smd[4]) + smd[6];
    uq = ((smd[1] + smd[3]) + smd[5]) + smd[7];
    bad = smi[0] + smi[1] + smi[2] + smi[3];
    __syncthreads();
}

// one chunk [cb, cb + len) of a range: tensor_stats_stage1's walk (vector v of thread t = t, t + 256, ..., component c of vector v is chunk
// element 4 v + c - r) with the moments written back.  NORMS false (trust_index -1): w is not read, nothing is summed.
template <bool NORMS>
__device__ __forceinline__ void lamb_chunk(const float* __restrict__ w, const float* __restrict__ g, float* __restrict__ m,
                                           float* __restrict__ v, int64_t cb, int len, int phase, const lamb_consts& k, double (&wq)[4],
                                           double (&uq)[4], uint32_t& bad) {
    const int t = threadIdx.x;
    const int r = phase < 0 ? 0 : (int)((cb + phase) & 3);
    const int64_t base = cb - r;              // the element of vector 0, component 0: 16-byte aligned in all four arrays when phase >= 0
    const int nv = (len + r + 3) >> 2;
    constexpr int U = 2;
    for (int v0 = t; v0 < nv; v0 += 256 * U) {
        if (phase >= 0 && 4 * v0 >= r && 4 * (v0 + 256 * (U - 1)) + 4 - r <= len) {      // U whole vectors: every load issued first
            float4 wv[U], gv[U], mv[U], qv[U];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int64_t e = base + 4 * (int64_t)(v0 + 256 * u);
                if (NORMS) wv[u] = *reinterpret_cast<const float4*>(w + e);
                else wv[u] = make_float4(0.f, 0.f, 0.f, 0.f);
                gv[u] = *reinterpret_cast<const float4*>(g + e);
                mv[u] = *reinterpret_cast<const float4*>(m + e);
                qv[u] = *reinterpret_cast<const float4*>(v + e);
            }
#pragma unroll
            for (int u = 0; u < U; ++u) {
                lamb_moments_elem<NORMS>(wv[u].x, gv[u].x, mv[u].x, qv[u].x, k, wq[0], uq[0], bad);
                lamb_moments_elem<NORMS>(wv[u].y, gv[u].y, mv[u].y, qv[u].y, k, wq[1], uq[1], bad);
                lamb_moments_elem<NORMS>(wv[u].z, gv[u].z, mv[u].z, qv[u].z, k, wq[2], uq[2], bad);
                lamb_moments_elem<NORMS>(wv[u].w, gv[u].w, mv[u].w, qv[u].w, k, wq[3], uq[3], bad);
                const int64_t e = base + 4 * (int64_t)(v0 + 256 * u);
                *reinterpret_cast<float4*>(m + e) = mv[u];
                *reinterpret_cast<float4*>(v + e) = qv[u];
            }
            continue;
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int vi = v0 + 256 * u;
            if (vi >= nv) break;
            const int j0 = 4 * vi - r;        // the chunk index of component 0
            const int64_t e = base + 4 * (int64_t)vi;
            if (phase >= 0 && j0 >= 0 && j0 + 4 <= len) {
                const float4 wv = NORMS ? *reinterpret_cast<const float4*>(w + e) : make_float4(0.f, 0.f, 0.f, 0.f);
                const float4 gv = *reinterpret_cast<const float4*>(g + e);
                float4 mv = *reinterpret_cast<const float4*>(m + e), qv = *reinterpret_cast<const float4*>(v + e);
                lamb_moments_elem<NORMS>(wv.x, gv.x, mv.x, qv.x, k, wq[0], uq[0], bad);
                lamb_moments_elem<NORMS>(wv.y, gv.y, mv.y, qv.y, k, wq[1], uq[1], bad);
                lamb_moments_elem<NORMS>(wv.z, gv.z, mv.z, qv.z, k, wq[2], uq[2], bad);
                lamb_moments_elem<NORMS>(wv.w, gv.w, mv.w, qv.w, k, wq[3], uq[3], bad);
                *reinterpret_cast<float4*>(m + e) = mv;
                *reinterpret_cast<float4*>(v + e) = qv;
            } else {                          // the chunk's head or tail, or the arrays disagree in phase: only elements of the chunk are addressed
#pragma unroll
                for (int c = 0; c < 4; ++c)
                    if (j0 + c >= 0 && j0 + c < len) {
                        float mi = m[e + c], qi = v[e + c];
                        lamb_moments_elem<NORMS>(NORMS ? w[e + c] : 0.f, g[e + c], mi, qi, k, wq[c], uq[c], bad);
                        m[e + c] = mi;
                        v[e + c] = qi;
                    }
            }
        }
    }
}

// one workgroup per chunk -> the moments of the chunk, and ws[chunk] where the range has a trust index.  st != nullptr: c1, c2 from the state.
__global__ __launch_bounds__(256) void lamb_moments_stage1(const float* __restrict__ w, const float* __restrict__ g, float* __restrict__ m,
                                                           float* __restrict__ v, lamb_table lt, float c1, float c2,
                                                           const vl_step_state* __restrict__ st, float eps, float clip_norm,
                                                           const float* __restrict__ sumsq, float gscale, const uint32_t* __restrict__ skip,
                                                           vl_lamb_row* __restrict__ ws) {
    __shared__ double sl[2][STAT_SLOTS];
    __shared__ uint32_t smi[4];
    if (skip && *skip) return;
    const int b = blockIdx.x, t = threadIdx.x;
    int s = 0;
    for (int k = 1; k < lt.n; ++k)
        if (lt.first[k] <= b) s = k;
    const int64_t cb = lt.r[s].begin + (int64_t)(b - lt.first[s]) * VL_STAT_CHUNK;
    const int64_t rest = lt.r[s].end - cb;
    const int len = rest < VL_STAT_CHUNK ? (int)rest : VL_STAT_CHUNK;
    const bool norms = lt.r[s].trust_index >= 0;
    const int phase = norms ? align_phase(w, g, m, v) : align_phase(g, m, v, nullptr);
    lamb_consts k;
    k.sc = clip_scale(clip_norm, sumsq, gscale);
    k.c1 = st ? __uint_as_float(st->reserved[VL_STEP_STATE_LAMB_C1]) : c1;
    k.c2 = st ? __uint_as_float(st->reserved[VL_STEP_STATE_LAMB_C2]) : c2;
    k.eps = eps;
    k.decay = lt.r[s].decay;
    double wq[4] = {0.0, 0.0, 0.0, 0.0}, uq[4] = {0.0, 0.0, 0.0, 0.0};
    uint32_t bad = 0u;
    if (!norms) {
        lamb_chunk<false>(w, g, m, v, cb, len, phase, k, wq, uq, bad);
        return;
    }
    lamb_chunk<true>(w, g, m, v, cb, len, phase, k, wq, uq, bad);
    const int r = phase < 0 ? 0 : (int)((cb + phase) & 3);
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        const int slot = (4 * t + c - r) & (STAT_SLOTS - 1);
        sl[0][slot] = wq[c];
        sl[1][slot] = uq[c];
    }
    __syncthreads();
    double wt = ((sl[0][4 * t] + sl[0][4 * t + 1]) + sl[0][4 * t + 2]) + sl[0][4 * t + 3];
    double ut = ((sl[1][4 * t] + sl[1][4 * t + 1]) + sl[1][4 * t + 2]) + sl[1][4 * t + 3];
    __syncthreads();
    lamb_block_reduce(wt, ut, bad, &sl[0][0], smi);
    if (t == 0) {
        vl_lamb_row row;
        row.w_sumsq = wt;
        row.u_sumsq = ut;
        row.nonfinite = bad;
        row.reserved = 0u;
        ws[b] = row;
    }
}

// one workgroup per range: its chunk rows in the order row t, t + 256, ... per thread, then the block's tree -> rows[index], trust[index]
__global__ __launch_bounds__(256) void lamb_moments_stage2(const vl_lamb_row* __restrict__ ws, lamb_table lt, const uint32_t* __restrict__ skip,
                                                           vl_lamb_row* __restrict__ rows, float* __restrict__ trust) {
#pragma clang fp contract(off)
    __shared__ double smd[8];
    __shared__ uint32_t smi[4];
    if (skip && *skip) return;
    const int s = blockIdx.x, idx = lt.r[s].trust_index;
    if (idx < 0) return;
    double wt = 0.0, ut = 0.0;
    uint32_t bad = 0u;
    for (int i = lt.first[s] + (int)threadIdx.x; i < lt.first[s + 1]; i += 256) {
        const vl_lamb_row r = ws[i];
        wt += r.w_sumsq;
        ut += r.u_sumsq;
        bad += r.nonfinite;
    }
    lamb_block_reduce(wt, ut, bad, smd, smi);
    if (threadIdx.x == 0) {
        vl_lamb_row row;
        row.w_sumsq = wt;
        row.u_sumsq = ut;
        row.nonfinite = bad;
        row.reserved = 0u;
        rows[idx] = row;
        const double wn = sqrt(wt), un = sqrt(ut);
        trust[idx] = (bad == 0u && wn > 0.0 && un > 0.0) ? (float)(wn / un) : 1.f;      // (a NaN norm fails > 0)
    }
}

static int lamb_scalars(const char* who, float c1, float c2, float eps, bool with_c) {
    VL_CHECK(eps > 0.f && eps <= 3.402823466e38f, "%s: eps must be finite and > 0, got %g", who, (double)eps);       // (NaN fails)
    if (with_c) {
        VL_CHECK(c1 >= 1.f && c1 <= 3.402823466e38f, "%s: c1 must be finite and >= 1, got %g", who, (double)c1);
        VL_CHECK(c2 >= 1.f && c2 <= 3.402823466e38f, "%s: c2 must be finite and >= 1, got %g", who, (double)c2);
    }
    return 0;
}

static int lamb_moments_launch(const char* who, const float* w, const float* g, float* m, float* v, int64_t count, float c1, float c2,
                               const vl_step_state* state, float eps, float clip_norm, const float* sumsq, float gscale, const uint32_t* skip,
                               const vl_lamb_range* ranges, int n_ranges, vl_lamb_row* rows, float* trust, int n_trust, void* ws,
                               size_t ws_bytes, vl_stream_t stream) {
    VL_CHECK(w, "%s: w is null", who);
    VL_CHECK(g, "%s: g is null", who);
    VL_CHECK(m, "%s: m is null", who);
    VL_CHECK(v, "%s: v is null", who);
    VL_CHECK(count > 0, "%s: count must be > 0, got %lld", who, (long long)count);
    VL_CHECK(n_trust >= 0 && ((rows && trust) || n_trust == 0), "%s: rows / trust: %d entries at a null pointer", who, n_trust);
    VL_CHECK(ws, "%s: ws is null", who);
    VL_CHECK((((uintptr_t)w | (uintptr_t)g | (uintptr_t)m | (uintptr_t)v | (uintptr_t)trust) & 3) == 0 &&
                 (((uintptr_t)rows | (uintptr_t)ws) & 7) == 0, "%s: misaligned pointer", who);
    if (int rc = lamb_scalars(who, c1, c2, eps, state == nullptr)) return rc;
    lamb_table lt;
    if (int rc = lamb_table_make(who, ranges, n_ranges, count, n_trust, &lt)) return rc;
    const size_t need = (size_t)lt.first[lt.n] * sizeof(vl_lamb_row);
    VL_CHECK(ws_bytes >= need, "%s: ws has %zu bytes, this table needs %zu (vl_lamb_moments_ws_bytes)", who, ws_bytes, need);
    hipLaunchKernelGGL(lamb_moments_stage1, dim3(lt.first[lt.n]), dim3(256), 0, (hipStream_t)stream, w, g, m, v, lt, c1, c2, state, eps,
                       clip_norm, sumsq, gscale, skip, reinterpret_cast<vl_lamb_row*>(ws));
    VL_LAUNCH_CHECK();
    hipLaunchKernelGGL(lamb_moments_stage2, dim3(lt.n), dim3(256), 0, (hipStream_t)stream, reinterpret_cast<const vl_lamb_row*>(ws), lt, skip,
                       rows, trust);
    VL_LAUNCH_CHECK();
    return 0;
}

extern "C" size_t vl_lamb_moments_ws_bytes(const vl_lamb_range* ranges, int n_ranges) {
    lamb_table lt;
    if (lamb_table_make("vl_lamb_moments_ws_bytes", ranges, n_ranges, -1, 0, &lt)) return 0;
    return (size_t)lt.first[lt.n] * sizeof(vl_lamb_row);
}

extern "C" int vl_lamb_moments(const float* w, const float* g, float* m, float* v, int64_t count, float c1, float c2, float eps,
                               float clip_norm, const float* sumsq, float gscale, const uint32_t* skip, const vl_lamb_range* ranges,
                               int n_ranges, vl_lamb_row* rows, float* trust, int n_trust, void* ws, size_t ws_bytes, vl_stream_t stream) {
    return lamb_moments_launch("vl_lamb_moments", w, g, m, v, count, c1, c2, nullptr, eps, clip_norm, sumsq, gscale, skip, ranges, n_ranges,
                               rows, trust, n_trust, ws, ws_bytes, stream);
}

extern "C" int vl_lamb_moments_st(const float* w, const float* g, float* m, float* v, int64_t count, const vl_step_state* state, float eps,
                                  float clip_norm, const float* sumsq, float gscale, const uint32_t* skip, const vl_lamb_range* ranges,
                                  int n_ranges, vl_lamb_row* rows, float* trust, int n_trust, void* ws, size_t ws_bytes,
                                  vl_stream_t stream) {
    VL_CHECK(state, "vl_lamb_moments_st: state is null");
    return lamb_moments_launch("vl_lamb_moments_st", w, g, m, v, count, 1.f, 1.f, state, eps, clip_norm, sumsq, gscale, skip, ranges,
                               n_ranges, rows, trust, n_trust, ws, ws_bytes, stream);
}

__device__ __forceinline__ void lamb_apply_elem(float& w, float m, float v, float a, float c1, float c2, float eps, float decay) {
#pragma clang fp contract(off)
    w = __builtin_fmaf(-a, lamb_dir(w, m, v, c1, c2, eps, decay), w);
}

// st != nullptr: lr, c1, c2 from the state.  The trust value is one uniform load per range.
__global__ void lamb_apply_kernel(float* __restrict__ w, const float* __restrict__ m, const float* __restrict__ v, lamb_table lt,
                                  const float* __restrict__ trust, float lr, float c1, float c2, const vl_step_state* __restrict__ st,
                                  float eps, const uint32_t* __restrict__ skip) {
#pragma clang fp contract(off)
    if (skip && *skip) return;
    if (st) {
        lr = st->lr;
        c1 = __uint_as_float(st->reserved[VL_STEP_STATE_LAMB_C1]);
        c2 = __uint_as_float(st->reserved[VL_STEP_STATE_LAMB_C2]);
    }
    const int64_t i0 = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, step = (int64_t)gridDim.x * blockDim.x;
    const int phase = align_phase(w, m, v, nullptr);
    for (int k = 0; k < lt.n; ++k) {
        const int ti = lt.r[k].trust_index;
        const float a = (lr * lt.r[k].lr_mult) * (ti < 0 ? 1.f : trust[ti]);
        const float decay = lt.r[k].decay;
        range_walk(lt.r[k].begin, lt.r[k].end, phase, i0, step, [&](int64_t i) { lamb_apply_elem(w[i], m[i], v[i], a, c1, c2, eps, decay); },
                   [&](int64_t v0, int64_t i) {
                       float4 wv = vec4(w, v0, i);
                       const float4 mv = vec4(m, v0, i), qv = vec4(v, v0, i);
                       lamb_apply_elem(wv.x, mv.x, qv.x, a, c1, c2, eps, decay);
                       lamb_apply_elem(wv.y, mv.y, qv.y, a, c1, c2, eps, decay);
                       lamb_apply_elem(wv.z, mv.z, qv.z, a, c1, c2, eps, decay);
                       lamb_apply_elem(wv.w, mv.w, qv.w, a, c1, c2, eps, decay);
                       vec4(w, v0, i) = wv;
                   });
    }
}

static int lamb_apply_launch(const char* who, float* w, const float* m, const float* v, int64_t count, float lr, float c1, float c2,
                             const vl_step_state* state, float eps, const uint32_t* skip, const vl_lamb_range* ranges, int n_ranges,
                             const float* trust, int n_trust, vl_stream_t stream) {
    VL_CHECK(w, "%s: w is null", who);
    VL_CHECK(m, "%s: m is null", who);
    VL_CHECK(v, "%s: v is null", who);
    VL_CHECK(count > 0, "%s: count must be > 0, got %lld", who, (long long)count);
    VL_CHECK(n_trust >= 0 && (trust || n_trust == 0), "%s: trust: %d entries at a null pointer", who, n_trust);
    if (int rc = lamb_scalars(who, c1, c2, eps, state == nullptr)) return rc;
    lamb_table lt;
    if (int rc = lamb_table_make(who, ranges, n_ranges, count, n_trust, &lt)) return rc;
    hipLaunchKernelGGL(lamb_apply_kernel, dim3(grid_for(count, 256, 4096)), dim3(256), 0, (hipStream_t)stream, w, m, v, lt, trust, lr, c1, c2,
                       state, eps, skip);
    VL_LAUNCH_CHECK();
    return 0;
}

extern "C" int vl_lamb_apply(float* w, const float* m, const float* v, int64_t count, float lr, float c1, float c2, float eps,
                             const uint32_t* skip, const vl_lamb_range* ranges, int n_ranges, const float* trust, int n_trust,
                             vl_stream_t stream) {
    return lamb_apply_launch("vl_lamb_apply", w, m, v, count, lr, c1, c2, nullptr, eps, skip, ranges, n_ranges, trust, n_trust, stream);
}

extern "C" int vl_lamb_apply_st(float* w, const float* m, const float* v, int64_t count, const vl_step_state* state, float eps,
                                const uint32_t* skip, const vl_lamb_range* ranges, int n_ranges, const float* trust, int n_trust,
                                vl_stream_t stream) {
    VL_CHECK(state, "vl_lamb_apply_st: state is null");
    return lamb_apply_launch("vl_lamb_apply_st", w, m, v, count, 0.f, 1.f, 1.f, state, eps, skip, ranges, n_ranges, trust, n_trust, stream);
}

// LAMB's two bias corrections: words of their own, written by a launch of their own (every other setter leaves them alone)
__global__ void step_state_set_lamb_kernel(vl_step_state* __restrict__ st, float c1, float c2) {
    st->reserved[VL_STEP_STATE_LAMB_C1] = __float_as_uint(c1);
    st->reserved[VL_STEP_STATE_LAMB_C2] = __float_as_uint(c2);
}

extern "C" int vl_step_state_set_lamb(vl_step_state* state, float c1, float c2, vl_stream_t stream) {
    VL_CHECK(state, "vl_step_state_set_lamb: state is null");
    if (int rc = lamb_scalars("vl_step_state_set_lamb", c1, c2, 1.f, true)) return rc;
    hipLaunchKernelGGL(step_state_set_lamb_kernel, dim3(1), dim3(1), 0, (hipStream_t)stream, state, c1, c2);
    VL_LAUNCH_CHECK();
    return 0;
}

__global__ void fill_kernel(float* __restrict__ p, int64_t count, float value) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < count; i += (int64_t)gridDim.x * blockDim.x) p[i] = value;
}

// ReluGrad in place (tf.nn.relu's gradient: 0 where the forward output is <= 0): d[i] = y[i] > 0 ? d[i] : 0
__global__ void relu_grad_kernel(float* __restrict__ d, const float* __restrict__ y, int64_t count) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < count; i += (int64_t)gridDim.x * blockDim.x)
        d[i] = y[i] > 0.f ? d[i] : 0.f;
}

extern "C" int vl_relu_grad(float* d, const float* y, int64_t count, vl_stream_t stream) {
    VL_CHECK(d && y && count > 0, "vl_relu_grad: bad argument");
    hipLaunchKernelGGL(relu_grad_kernel, dim3(grid_for(count, 256, 4096)), dim3(256), 0, (hipStream_t)stream, d, y, count);
    VL_LAUNCH_CHECK();
    return 0;
}

// ---- dropout on the ReLU'd fc layers of the tower (fc6 / fc7), in place, no mask buffer (vltf.h: vl_fc_dropout_fwd) -----------------
// The draw of element e is a function of (seed, salt, e) alone: the scalar head / tail and the 16-byte interior call one element
// function with the element's index relative to the pointer given, so neither the launch geometry nor the alignment changes a mask.
__device__ __forceinline__ uint64_t fc_dropout_stream(uint64_t seed, uint32_t salt) {
    return seed ^ splitmix64(0xFC00ull + (uint64_t)salt);
}

__device__ __forceinline__ float fc_dropout_elem(float y, uint64_t s, int64_t e, float keep) {
#pragma clang fp contract(off)
    const uint64_t h = splitmix64(s ^ splitmix64((uint64_t)e));
    const float uni = (float)(h >> 40) * (1.0f / 16777216.0f);
    return uni < keep ? y / keep : 0.f;
}

__device__ __forceinline__ void fc_dropout_body(float* __restrict__ y, int64_t count, float keep, uint64_t s, int64_t i0, int64_t step) {
    range_walk(0, count, align_phase(y, nullptr, nullptr, nullptr), i0, step, [&](int64_t e) { y[e] = fc_dropout_elem(y[e], s, e, keep); },
               [&](int64_t v0, int64_t i) {
                   const int64_t e = v0 + 4 * i;
                   float4 v = vec4(y, v0, i);
                   v.x = fc_dropout_elem(v.x, s, e, keep);
                   v.y = fc_dropout_elem(v.y, s, e + 1, keep);
                   v.z = fc_dropout_elem(v.z, s, e + 2, keep);
                   v.w = fc_dropout_elem(v.w, s, e + 3, keep);
                   vec4(y, v0, i) = v;
               });
}

__global__ __launch_bounds__(256) void fc_dropout_fwd_kernel(float* __restrict__ y, int64_t count, float keep, uint64_t seed, uint32_t salt) {
    fc_dropout_body(y, count, keep, fc_dropout_stream(seed, salt), (int64_t)blockIdx.x * blockDim.x + threadIdx.x,
                    (int64_t)gridDim.x * blockDim.x);
}

// the seed as vl_dropout_fwd_st forms it, from the step state when the kernel runs (a replayed step's own count)
__global__ __launch_bounds__(256) void fc_dropout_fwd_st_kernel(float* __restrict__ y, int64_t count, float keep,
                                                                const vl_step_state* __restrict__ st, uint32_t salt) {
    fc_dropout_body(y, count, keep, fc_dropout_stream(((uint64_t)st->step << 20) ^ 0x5DEECE66Dull, salt),
                    (int64_t)blockIdx.x * blockDim.x + threadIdx.x, (int64_t)gridDim.x * blockDim.x);
}

// a lane takes 4 elements per pass: the grid covers 4 * 256 * VL_FC_DROPOUT_GRID_CAP elements before its loop turns
#define VL_FC_DROPOUT_GRID_CAP 4096

extern "C" int vl_fc_dropout_fwd(float* y, int64_t count, float keep, uint64_t seed, uint32_t salt, vl_stream_t stream) {
    VL_CHECK(y && ((uintptr_t)y & 3) == 0 && count > 0 && keep > 0.f && keep <= 1.f, "vl_fc_dropout_fwd: bad argument");
    hipLaunchKernelGGL(fc_dropout_fwd_kernel, dim3(grid_for((count + 3) / 4, 256, VL_FC_DROPOUT_GRID_CAP)), dim3(256), 0,
                       (hipStream_t)stream, y, count, keep, seed, salt);
    VL_LAUNCH_CHECK();
    return 0;
}

extern "C" int vl_fc_dropout_fwd_st(float* y, int64_t count, float keep, const vl_step_state* state, uint32_t salt,
                                    vl_stream_t stream) {
    VL_CHECK(y && ((uintptr_t)y & 3) == 0 && state && count > 0 && keep > 0.f && keep <= 1.f, "vl_fc_dropout_fwd_st: bad argument");
    hipLaunchKernelGGL(fc_dropout_fwd_st_kernel, dim3(grid_for((count + 3) / 4, 256, VL_FC_DROPOUT_GRID_CAP)), dim3(256), 0,
                       (hipStream_t)stream, y, count, keep, state, salt);
    VL_LAUNCH_CHECK();
    return 0;
}

// ReluGrad and the dropout's gradient in one: y is the dropped ReLU output, > 0 exactly where the ReLU was active and the draw kept
__device__ __forceinline__ float relu_dropout_grad_elem(float d, float y, float keep) {
#pragma clang fp contract(off)
    return y > 0.f ? d / keep : 0.f;
}

__global__ __launch_bounds__(256) void relu_dropout_grad_kernel(float* __restrict__ d, const float* __restrict__ y, int64_t count, float keep) {
    const int64_t i0 = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, step = (int64_t)gridDim.x * blockDim.x;
    range_walk(0, count, align_phase(d, y, nullptr, nullptr), i0, step, [&](int64_t e) { d[e] = relu_dropout_grad_elem(d[e], y[e], keep); },
               [&](int64_t v0, int64_t i) {
                   float4 dv = vec4(d, v0, i);
                   const float4 yv = vec4(y, v0, i);
                   dv.x = relu_dropout_grad_elem(dv.x, yv.x, keep);
                   dv.y = relu_dropout_grad_elem(dv.y, yv.y, keep);
                   dv.z = relu_dropout_grad_elem(dv.z, yv.z, keep);
                   dv.w = relu_dropout_grad_elem(dv.w, yv.w, keep);
                   vec4(d, v0, i) = dv;
               });
}

extern "C" int vl_relu_dropout_grad(float* d, const float* y, int64_t count, float keep, vl_stream_t stream) {
    VL_CHECK(d && y && (((uintptr_t)d | (uintptr_t)y) & 3) == 0 && count > 0 && keep > 0.f && keep <= 1.f,
             "vl_relu_dropout_grad: bad argument");
    hipLaunchKernelGGL(relu_dropout_grad_kernel, dim3(grid_for((count + 3) / 4, 256, VL_FC_DROPOUT_GRID_CAP)), dim3(256), 0,
                       (hipStream_t)stream, d, y, count, keep);
    VL_LAUNCH_CHECK();
    return 0;
}

extern "C" int vl_fill(float* p, int64_t count, float value, vl_stream_t stream) {
    VL_CHECK(p && count > 0, "vl_fill: bad argument");
    hipLaunchKernelGGL(fill_kernel, dim3(grid_for(count, 256, 4096)), dim3(256), 0, (hipStream_t)stream, p, count, value);
    VL_LAUNCH_CHECK();
    return 0;
}

// ---- tensor-list plumbing of multi-input pipelines (tf_util.py:99-192) ----------------------------------------------------------
// concat / vec_seq_concat / ibias / replicate_auxilliary_tensor are all strided block copies; avg / maximum are elementwise.
__global__ void copy2d_kernel(const float* __restrict__ src, int64_t src_ld, float* __restrict__ dst, int64_t dst_ld, int rows,
                              int cols) {
    const int64_t total = (int64_t)rows * cols;
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (int64_t)gridDim.x * blockDim.x) {
        const int64_t r = e / cols, c = e - r * cols;
        dst[r * dst_ld + c] = src[r * src_ld + c];
    }
}

extern "C" int vl_copy2d(const float* src, int64_t src_ld, float* dst, int64_t dst_ld, int rows, int cols, vl_stream_t stream) {
    VL_CHECK(src && dst && rows > 0 && cols > 0 && src_ld >= 0 && dst_ld >= cols, "vl_copy2d: bad argument");
    hipLaunchKernelGGL(copy2d_kernel, dim3(grid_for((int64_t)rows * cols, 256, 4096)), dim3(256), 0, (hipStream_t)stream, src, src_ld, dst,
                       dst_ld, rows, cols);
    VL_LAUNCH_CHECK();
    return 0;
}

// op 0: out = a + b;  1: out = (a + b) / 2 (tf.reduce_mean over two inputs);  2: out = max(a, b) (tf.reduce_max)
__global__ void eltwise2_kernel(const float* __restrict__ a, const float* __restrict__ b, float* __restrict__ out, int64_t count, int op) {
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < count; e += (int64_t)gridDim.x * blockDim.x) {
        const float x = a[e], y = b[e];
        out[e] = op == 0 ? x + y : (op == 1 ? (x + y) * 0.5f : fmaxf(x, y));
    }
}

extern "C" int vl_eltwise2(const float* a, const float* b, float* out, int64_t count, int op, vl_stream_t stream) {
    VL_CHECK(a && b && out && count > 0 && op >= 0 && op <= 2, "vl_eltwise2: bad argument");
    hipLaunchKernelGGL(eltwise2_kernel, dim3(grid_for(count, 256, 4096)), dim3(256), 0, (hipStream_t)stream, a, b, out, count, op);
    VL_LAUNCH_CHECK();
    return 0;
}

// gradient of max(a, b) as tf.reduce_max registers it (_MinOrMaxGrad): the inputs equal to the maximum share the gradient evenly
// (two ReLU outputs that are both 0 tie all the time)
__global__ void max2_grad_kernel(const float* __restrict__ a, const float* __restrict__ b, const float* __restrict__ d,
                                 float* __restrict__ da, float* __restrict__ db, int64_t count) {
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < count; e += (int64_t)gridDim.x * blockDim.x) {
        const float x = a[e], y = b[e], g = d[e];
        da[e] = x > y ? g : (x == y ? 0.5f * g : 0.f);
        db[e] = y > x ? g : (x == y ? 0.5f * g : 0.f);
    }
}

extern "C" int vl_max2_grad(const float* a, const float* b, const float* d, float* da, float* db, int64_t count, vl_stream_t stream) {
    VL_CHECK(a && b && d && da && db && count > 0, "vl_max2_grad: bad argument");
    hipLaunchKernelGGL(max2_grad_kernel, dim3(grid_for(count, 256, 4096)), dim3(256), 0, (hipStream_t)stream, a, b, d, da, db, count);
    VL_LAUNCH_CHECK();
    return 0;
}

// apply_tensor_list_fusion avg | maximum over a LIST of equally shaped tensors (tf.reduce_mean / tf.reduce_max over axis 0 of the
// stacked list, tf_util.py:142-145) and its gradient.  The pointer lists are host arrays, passed to the kernel by value.
static constexpr int FUSE_MAX = 8;
struct FuseList { const float* in[FUSE_MAX]; float* din[FUSE_MAX]; int n; };

__global__ void fuse_n_kernel(const FuseList l, float* __restrict__ out, int64_t count, int op) {
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < count; e += (int64_t)gridDim.x * blockDim.x) {
        float acc = l.in[0][e];
        for (int i = 1; i < l.n; ++i) acc = op == 0 ? acc + l.in[i][e] : fmaxf(acc, l.in[i][e]);
        out[e] = op == 0 ? acc / (float)l.n : acc;
    }
}

// avg: every input gets d / n; maximum: the inputs equal to the maximum share d evenly (tf _MinOrMaxGrad); din[i] == null is skipped
__global__ void fuse_n_grad_kernel(const FuseList l, const float* __restrict__ d, int64_t count, int op) {
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < count; e += (int64_t)gridDim.x * blockDim.x) {
        const float g = d[e];
        if (op == 0) {
            for (int i = 0; i < l.n; ++i)
                if (l.din[i]) l.din[i][e] = g / (float)l.n;
        } else {
            float m = l.in[0][e];
            for (int i = 1; i < l.n; ++i) m = fmaxf(m, l.in[i][e]);
            int hits = 0;
            for (int i = 0; i < l.n; ++i) hits += l.in[i][e] == m;
            for (int i = 0; i < l.n; ++i)
                if (l.din[i]) l.din[i][e] = l.in[i][e] == m ? g / (float)hits : 0.f;
        }
    }
}

extern "C" int vl_fuse_n(const float* const* ins, int n, float* out, int64_t count, int op, vl_stream_t stream) {
    VL_CHECK(ins && out && n >= 1 && n <= FUSE_MAX && count > 0 && (op == 0 || op == 1), "vl_fuse_n: bad argument (1..8 inputs, op 0 avg | 1 maximum)");
    FuseList l = {};
    l.n = n;
    for (int i = 0; i < n; ++i) {
        VL_CHECK(ins[i], "vl_fuse_n: null input");
        l.in[i] = ins[i];
    }
    hipLaunchKernelGGL(fuse_n_kernel, dim3(grid_for(count, 256, 4096)), dim3(256), 0, (hipStream_t)stream, l, out, count, op);
    VL_LAUNCH_CHECK();
    return 0;
}

extern "C" int vl_fuse_n_grad(const float* const* ins, int n, const float* d, float* const* dins, int64_t count, int op, vl_stream_t stream) {
    VL_CHECK(d && dins && n >= 1 && n <= FUSE_MAX && count > 0 && (op == 0 || op == 1), "vl_fuse_n_grad: bad argument");
    VL_CHECK(op == 0 || ins, "vl_fuse_n_grad: the maximum needs the inputs");
    FuseList l = {};
    l.n = n;
    for (int i = 0; i < n; ++i) {
        if (op == 1) {
            VL_CHECK(ins[i], "vl_fuse_n_grad: null input");
            l.in[i] = ins[i];
        }
        l.din[i] = dins[i];
    }
    hipLaunchKernelGGL(fuse_n_grad_kernel, dim3(grid_for(count, 256, 4096)), dim3(256), 0, (hipStream_t)stream, l, d, count, op);
    VL_LAUNCH_CHECK();
    return 0;
}
