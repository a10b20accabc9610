"""Thin torch-tensor wrappers over the C-ABI (include/vltf.h).  Tensors are device allocations
only: every wrapper passes ``data_ptr()`` and the current HIP stream; no torch math runs here."""
import ctypes as C
import math

import numpy as np
import torch

from . import _ffi

F32 = torch.float32


def stream():
    return torch.cuda.current_stream().cuda_stream


def _p(t):
    return None if t is None else t.data_ptr()


def _f32(*ts):
    for t in ts:
        if t is None:
            continue
        if not (t.is_cuda and t.dtype == F32):
            raise _ffi.VltfError("expected a CUDA/HIP float32 tensor, got %s on %s" % (t.dtype, t.device))


def _dense(*ts):
    for t in ts:
        if t is not None and not t.is_contiguous():
            raise _ffi.VltfError("expected a contiguous tensor")


# ---- input ---------------------------------------------------------------------------------------
def phase_split_shape(n, c, h, w, halo, phase):
    """Shape of an activation tensor with a zero halo, plain (phase 1) or column-phase-split (vl_conv_set_x_phase_split)."""
    if phase <= 1:
        return (n, c, h + 2 * halo, w + 2 * halo)
    return (n, c * phase, h + 2 * halo, -(-(w + 2 * halo) // phase))


def input_prep_u8(src, dst, crop_y=None, crop_x=None, mirror=None, mean_bgr=None, halo=0, phase=1, out_hw=None):
    """src uint8 [n, raw_h, raw_w, 3] (HWC, BGR) -> dst f32 [n, 3, out_h + 2 halo, out_w + 2 halo] (dataset_.py:481-501);
    phase > 1: dst is phase_split_shape(n, 3, *out_hw, halo, phase) and out_hw must be given."""
    if src.dtype != torch.uint8 or not src.is_cuda:
        raise _ffi.VltfError("input_prep_u8: src must be a device uint8 tensor")
    _f32(dst, mean_bgr)
    _dense(src, dst, crop_y, crop_x, mirror, mean_bgr)
    n, rh, rw, c = src.shape
    if out_hw is None:
        if phase > 1:
            raise _ffi.VltfError("input_prep_u8: out_hw is required with a phase-split destination")
        out_hw = (dst.shape[2] - 2 * halo, dst.shape[3] - 2 * halo)
    if c != 3 or tuple(dst.shape) != phase_split_shape(n, 3, out_hw[0], out_hw[1], halo, phase):
        raise _ffi.VltfError("input_prep_u8: shape mismatch %s -> %s" % (tuple(src.shape), tuple(dst.shape)))
    _ffi.call("vl_input_prep_u8", _p(src), _p(dst), n, rh, rw, out_hw[0], out_hw[1], _p(crop_y), _p(crop_x), _p(mirror),
              _p(mean_bgr), halo, phase, stream())


def _check_box(who, box, mirror, n):
    """box int32 [n, 4] and mirror uint8 [n] (or None), contiguous on the device: what the box kernels read per frame."""
    if not torch.is_tensor(box) or not box.is_cuda or box.dtype != torch.int32 or tuple(box.shape) != (n, 4) or not box.is_contiguous():
        raise _ffi.VltfError("%s: box must be a contiguous device int32 [%d, 4] tensor (y0, x0, bh, bw per frame)" % (who, n))
    if mirror is not None and (not mirror.is_cuda or mirror.dtype != torch.uint8 or mirror.numel() < n or not mirror.is_contiguous()):
        raise _ffi.VltfError("%s: mirror must be a contiguous device uint8 tensor of %d entries" % (who, n))


def input_prep_u8_box(src, dst, box, mirror=None, mean_bgr=None, halo=0, phase=1, out_hw=None):
    """Random resized crop (vl_input_prep_u8_box): frame i's box[i] = (y0, x0, bh, bw) of src uint8 [n, raw_h, raw_w, 3] is resampled
    bilinearly to out_hw, mirrored and mean-subtracted into dst, input_prep_u8's destination.  The kernel clamps every box into the frame."""
    if src.dtype != torch.uint8 or not src.is_cuda or src.dim() != 4:
        raise _ffi.VltfError("input_prep_u8_box: src must be a device uint8 [n, h, w, 3] tensor")
    _f32(dst, mean_bgr)
    _dense(src, dst, mean_bgr)
    n, rh, rw, c = src.shape
    _check_box("input_prep_u8_box", box, mirror, n)
    if out_hw is None:
        if phase > 1:
            raise _ffi.VltfError("input_prep_u8_box: out_hw is required with a phase-split destination")
        out_hw = (dst.shape[2] - 2 * halo, dst.shape[3] - 2 * halo)
    if c != 3 or tuple(dst.shape) != phase_split_shape(n, 3, out_hw[0], out_hw[1], halo, phase):
        raise _ffi.VltfError("input_prep_u8_box: shape mismatch %s -> %s" % (tuple(src.shape), tuple(dst.shape)))
    _ffi.call("vl_input_prep_u8_box", _p(src), _p(dst), n, rh, rw, out_hw[0], out_hw[1], _p(box), _p(mirror), _p(mean_bgr), halo, phase,
              stream())


def nhwc_to_nchw(src, dst, halo=0, phase=1):
    _f32(src, dst); _dense(src, dst)
    n, h, w, c = src.shape
    if tuple(dst.shape) != phase_split_shape(n, c, h, w, halo, phase):
        raise _ffi.VltfError("nhwc_to_nchw: shape mismatch %s -> %s (halo %d)" % (tuple(src.shape), tuple(dst.shape), halo))
    _ffi.call("vl_nhwc_to_nchw", _p(src), _p(dst), n, h, w, c, halo, phase, stream())


def nchw_to_nhwc(src, dst):
    _f32(src, dst); _dense(src, dst)
    n, c, h, w = src.shape
    _ffi.call("vl_nchw_to_nhwc", _p(src), _p(dst), n, c, h, w, stream())


# ---- convolution ---------------------------------------------------------------------------------
class Conv:
    """Descriptor for one dcnn.conv layer (alexnet.py:15-31): TF 'SAME' conv per group."""

    def __init__(self, cin, h, w, cout, kh, kw, stride, groups):
        self.cin, self.h, self.w, self.cout = cin, h, w, cout
        self.kh, self.kw, self.stride, self.groups = kh, kw, stride, groups
        self._d = C.c_void_p()
        _ffi.check(_ffi.lib().vl_conv_create(C.byref(self._d), cin, h, w, cout, kh, kw, stride, groups), "vl_conv_create")
        oh, ow = C.c_int(), C.c_int()
        _ffi.check(_ffi.lib().vl_conv_out_hw(self._d, C.byref(oh), C.byref(ow)), "vl_conv_out_hw")
        self.oh, self.ow = oh.value, ow.value
        self.w_shape = (kh, kw, cin // groups, cout)
        self.x_halo = self.y_halo = self.dy_halo = self.dx_halo = 0

    def same_pad(self):
        """Largest SAME padding on any side (TF rule): the halo that makes the gather test-free."""
        def one(n, k, s):
            out = -(-n // s)
            tot = max((out - 1) * s + k - n, 0)
            return tot - tot // 2
        return max(one(self.h, self.kh, self.stride), one(self.w, self.kw, self.stride))

    def set_halo(self, x_halo=0, y_halo=0, dy_halo=0, dx_halo=0):
        """Declare the zero-halo layouts of x / y / dy / dx (include/vltf.h: vl_conv_set_halo)."""
        _ffi.call("vl_conv_set_halo", self._d, x_halo, y_halo, dy_halo, dx_halo)
        self.x_halo, self.y_halo, self.dy_halo, self.dx_halo = x_halo, y_halo, dy_halo, dx_halo
        self.x_phase = int(_ffi.lib().vl_conv_x_phase(self._d))

    def set_x_phase_split(self, on=True):
        """Store x column-phase-split (strided convs in the padded layout; include/vltf.h).  Returns the phase count."""
        _ffi.call("vl_conv_set_x_phase_split", self._d, int(on))
        self.x_phase = int(_ffi.lib().vl_conv_x_phase(self._d))
        return self.x_phase

    def _shape(self, n, c, h, w, halo):
        return (n, c, h + 2 * halo, w + 2 * halo)

    def x_shape(self, n):
        return phase_split_shape(n, self.cin, self.h, self.w, self.x_halo, getattr(self, "x_phase", 1))

    def __del__(self):
        try:
            if self._d:
                _ffi.lib().vl_conv_destroy(self._d)
                self._d = None
        except Exception:
            pass

    def fwd(self, x, w, bias, y, relu=True):
        _f32(x, w, bias, y); _dense(x, w, bias, y)
        n = x.shape[0]
        if tuple(x.shape) != self.x_shape(n) or tuple(y.shape) != self._shape(n, self.cout, self.oh, self.ow, self.y_halo):
            raise _ffi.VltfError("conv.fwd: shape mismatch x=%s y=%s (halos %d, %d)" % (tuple(x.shape), tuple(y.shape),
                                                                                        self.x_halo, self.y_halo))
        _ffi.call("vl_conv_fwd", self._d, _p(x), _p(w), _p(bias), _p(y), n, int(relu), stream())

    def wt_transpose(self, w, wt):
        _f32(w, wt); _dense(w, wt)
        _ffi.call("vl_conv_wt_transpose", self._d, _p(w), _p(wt), stream())

    def dgrad(self, dy, wt, dx, relu_mask=None):
        _f32(dy, wt, dx, relu_mask); _dense(dy, wt, dx, relu_mask)
        n = dy.shape[0]
        if tuple(dy.shape) != self._shape(n, self.cout, self.oh, self.ow, self.dy_halo) or \
                tuple(dx.shape) != self._shape(n, self.cin, self.h, self.w, self.dx_halo) or \
                (relu_mask is not None and tuple(relu_mask.shape) != self._shape(n, self.cin, self.h, self.w, self.x_halo)):
            raise _ffi.VltfError("conv.dgrad: shape mismatch dy=%s dx=%s" % (tuple(dy.shape), tuple(dx.shape)))
        _ffi.call("vl_conv_dgrad", self._d, _p(dy), _p(wt), _p(dx), _p(relu_mask), dy.shape[0], stream())

    def wgrad_ws_bytes(self, n):
        return int(_ffi.lib().vl_conv_wgrad_ws_bytes(self._d, n))

    def fuses_bias(self):
        return bool(_ffi.lib().vl_conv_wgrad_fuses_bias(self._d))

    def wgrad(self, x, dy, dw, ws, db=None):
        """dw (and, when fuses_bias(), db = sum of dy over n,h,w in the same pass)."""
        _f32(x, dy, dw, db); _dense(x, dy, dw, ws, db)
        n = x.shape[0]
        if tuple(x.shape) != self.x_shape(n) or tuple(dy.shape) != self._shape(n, self.cout, self.oh, self.ow, self.dy_halo):
            raise _ffi.VltfError("conv.wgrad: shape mismatch x=%s dy=%s" % (tuple(x.shape), tuple(dy.shape)))
        nbytes = 0 if ws is None else ws.numel() * ws.element_size()
        _ffi.call("vl_conv_wgrad", self._d, _p(x), _p(dy), _p(dw), _p(db), _p(ws), nbytes, x.shape[0], stream())


    # ---- the bf16 path: operands in the c8 layout [n][ceil(c/8)][h + 2 halo][w + 2 halo][8] bf16 (include/vltf.h) -------------
    def c8_w_bytes(self, bwd=False):
        return int(_ffi.lib().vl_conv_c8_w_bytes(self._d, int(bwd)))

    def c8_pack_w(self, w, wb, bwd=False):
        """HWIO fp32 weights -> packed bf16 operand of c8_fwd (bwd=False) / c8_dgrad (bwd=True); wb: uint8 tensor of c8_w_bytes."""
        _f32(w); _dense(w, wb)
        if wb.numel() * wb.element_size() < self.c8_w_bytes(bwd):
            raise _ffi.VltfError("conv.c8_pack_w: weight buffer too small")
        _ffi.call("vl_conv_c8_pack_w", self._d, _p(w), _p(wb), int(bwd), stream())

    def _c8_check(self, t, n, c, h, w, halo, what):
        if t is not None and (t.dtype != torch.bfloat16 or tuple(t.shape) != c8_shape(n, c, h, w, halo) or not t.is_contiguous()):
            raise _ffi.VltfError("conv: %s must be a contiguous bf16 c8 tensor %s, got %s %s" % (what, c8_shape(n, c, h, w, halo),
                                                                                                 t.dtype, tuple(t.shape)))

    def c8_fwd(self, xb, wb, bias, y=None, yb=None, relu=True):
        n = xb.shape[0]
        _f32(bias, y); _dense(bias, y, wb)
        self._c8_check(xb, n, self.cin, self.h, self.w, self.x_halo, "xb")
        self._c8_check(yb, n, self.cout, self.oh, self.ow, self.y_halo, "yb")
        if y is not None and tuple(y.shape) != self._shape(n, self.cout, self.oh, self.ow, self.y_halo):
            raise _ffi.VltfError("conv.c8_fwd: y shape %s" % (tuple(y.shape),))
        _ffi.call("vl_conv_c8_fwd", self._d, _p(xb), _p(wb), _p(bias), _p(y), _p(yb), n, int(relu), stream())

    def c8_dgrad(self, dyb, wbt, dx=None, dxb=None, relu_mask=None, relu_mask_c8=None):
        """relu_mask (fp32, dx's layout) or relu_mask_c8 (this layer's packed input xb): fused ReluGrad of the producing layer."""
        n = dyb.shape[0]
        self._c8_check(relu_mask_c8, n, self.cin, self.h, self.w, self.x_halo, "relu_mask_c8")
        _f32(dx, relu_mask); _dense(dx, relu_mask, wbt)
        self._c8_check(dyb, n, self.cout, self.oh, self.ow, self.dy_halo, "dyb")
        self._c8_check(dxb, n, self.cin, self.h, self.w, self.dx_halo, "dxb")
        for t in (dx, relu_mask):
            if t is not None and tuple(t.shape) != self._shape(n, self.cin, self.h, self.w, self.dx_halo):
                raise _ffi.VltfError("conv.c8_dgrad: dx / relu_mask shape %s" % (tuple(t.shape),))
        _ffi.call("vl_conv_c8_dgrad", self._d, _p(dyb), _p(wbt), _p(dx), _p(dxb), _p(relu_mask), _p(relu_mask_c8), n, stream())

    # a strided first layer as a stride-1 layer over its space-to-depth input (include/vltf.h: vl_s2d_*)
    def s2d_layer(self):
        """Descriptor of the equivalent stride-1 layer (halos 1 for x and dy, dense y)."""
        s, ka = self.stride, (self.kh - 1) // self.stride + 1
        eq = Conv(self.cin * s * s, self.oh, self.ow, self.cout, ka, ka, 1, 1)
        eq.set_halo((ka - 1) // 2, 0, (ka - 1) // 2, 0)
        return eq

    def s2d_c8_from_x0(self, x0, xb):
        _f32(x0); _dense(x0, xb)
        n = x0.shape[0]
        s, ka = self.stride, (self.kh - 1) // self.stride + 1
        if tuple(x0.shape) != self.x_shape(n) or xb.dtype != torch.bfloat16 or \
                tuple(xb.shape) != c8_shape(n, self.cin * s * s, self.oh, self.ow, (ka - 1) // 2):
            raise _ffi.VltfError("conv.s2d_c8_from_x0: shape mismatch x0=%s xb=%s" % (tuple(x0.shape), tuple(xb.shape)))
        _ffi.call("vl_s2d_c8_from_x0", self._d, _p(x0), _p(xb), n, stream())

    def input_prep_u8_s2d(self, src, xb, crop_y=None, crop_x=None, mirror=None, mean_bgr=None):
        """uint8 frames [n, raw_h, raw_w, 3] -> the packed space-to-depth input (= input_prep_u8 + s2d_c8_from_x0)."""
        if src.dtype != torch.uint8 or not src.is_cuda or src.dim() != 4 or src.shape[3] != self.cin:
            raise _ffi.VltfError("conv.input_prep_u8_s2d: src must be a device uint8 [n, h, w, %d] tensor" % self.cin)
        _f32(mean_bgr); _dense(src, xb, mean_bgr)
        n = src.shape[0]
        s, ka = self.stride, (self.kh - 1) // self.stride + 1
        if xb.dtype != torch.bfloat16 or tuple(xb.shape) != c8_shape(n, self.cin * s * s, self.oh, self.ow, (ka - 1) // 2):
            raise _ffi.VltfError("conv.input_prep_u8_s2d: xb shape %s" % (tuple(xb.shape),))
        for t, dt in ((crop_y, torch.int32), (crop_x, torch.int32), (mirror, torch.uint8)):
            if t is not None and (t.dtype != dt or t.numel() < n or not t.is_contiguous()):
                raise _ffi.VltfError("conv.input_prep_u8_s2d: crop / mirror must be contiguous int32 / uint8 tensors of n entries")
        _ffi.call("vl_input_prep_u8_s2d", self._d, _p(src), _p(xb), n, src.shape[1], src.shape[2], _p(crop_y), _p(crop_x), _p(mirror),
                  _p(mean_bgr), stream())

    def input_prep_u8_box_s2d(self, src, xb, box, mirror=None, mean_bgr=None):
        """Random resized crop into the packed space-to-depth input (= input_prep_u8_box + s2d_c8_from_x0, bit for bit)."""
        if src.dtype != torch.uint8 or not src.is_cuda or src.dim() != 4 or src.shape[3] != self.cin:
            raise _ffi.VltfError("conv.input_prep_u8_box_s2d: src must be a device uint8 [n, h, w, %d] tensor" % self.cin)
        _f32(mean_bgr); _dense(src, xb, mean_bgr)
        n = src.shape[0]
        s, ka = self.stride, (self.kh - 1) // self.stride + 1
        if xb.dtype != torch.bfloat16 or tuple(xb.shape) != c8_shape(n, self.cin * s * s, self.oh, self.ow, (ka - 1) // 2):
            raise _ffi.VltfError("conv.input_prep_u8_box_s2d: xb shape %s" % (tuple(xb.shape),))
        _check_box("conv.input_prep_u8_box_s2d", box, mirror, n)
        _ffi.call("vl_input_prep_u8_box_s2d", self._d, _p(src), _p(xb), n, src.shape[1], src.shape[2], _p(box), _p(mirror), _p(mean_bgr),
                  stream())

    def cutmix_pairs_s2d(self, xb, clips, fpc, box):
        """CutMix / VideoMix in place in the packed space-to-depth input (vl_cutmix_pairs_s2d): xb is what input_prep_u8_s2d writes
        for clips * fpc frames; the box (t0, t1, y0, y1, x0, x1) of the h x w frames is exchanged between clip i and clip
        clips - 1 - i bit for bit.  box: a 6-tuple or a six-int32 device tensor, as in ops.cutmix_pairs."""
        clips, fpc = int(clips), int(fpc)
        s, ka = self.stride, (self.kh - 1) // self.stride + 1
        if not torch.is_tensor(xb) or not xb.is_cuda or xb.dtype != torch.bfloat16 or not xb.is_contiguous() or \
                (clips >= 0 and fpc > 0 and tuple(xb.shape) != c8_shape(clips * fpc, self.cin * s * s, self.oh, self.ow, (ka - 1) // 2)):
            raise _ffi.VltfError("conv.cutmix_pairs_s2d: xb must be the contiguous bf16 packed input of %d clips of %d frames, got %s"
                                 % (clips, fpc, tuple(xb.shape) if torch.is_tensor(xb) else type(xb)))
        host, dev, keep = _cut_box(box, "conv.cutmix_pairs_s2d")
        _ffi.call("vl_cutmix_pairs_s2d", self._d, _p(xb), clips, fpc, host, dev, stream())
        del keep

    def erase_boxes_s2d(self, xb, clips, fpc, table, mode, scale):
        """Random erasing in place in the packed space-to-depth input (vl_erase_boxes_s2d): xb is what input_prep_u8_s2d writes for
        clips * fpc frames; clip i's box of the h x w frames is overwritten with the fill of `mode`, rounded to bf16.  table, mode,
        scale: as in ops.erase_boxes."""
        clips, fpc = int(clips), int(fpc)
        s, ka = self.stride, (self.kh - 1) // self.stride + 1
        if not torch.is_tensor(xb) or not xb.is_cuda or xb.dtype != torch.bfloat16 or not xb.is_contiguous() or \
                (clips >= 0 and fpc > 0 and tuple(xb.shape) != c8_shape(clips * fpc, self.cin * s * s, self.oh, self.ow, (ka - 1) // 2)):
            raise _ffi.VltfError("conv.erase_boxes_s2d: xb must be the contiguous bf16 packed input of %d clips of %d frames, got %s"
                                 % (clips, fpc, tuple(xb.shape) if torch.is_tensor(xb) else type(xb)))
        _erase_table(table, clips, "conv.erase_boxes_s2d")
        _ffi.call("vl_erase_boxes_s2d", self._d, _p(xb), clips, fpc, _p(table), int(mode), float(scale), stream())

    def s2d_weights(self, src, dst, grad=False):
        """grad=False: w [k][k][cin][cout] -> [ka][ka][cin s^2][cout]; grad=True: the stride-1 layer's dw -> dw."""
        _f32(src, dst); _dense(src, dst)
        s, ka = self.stride, (self.kh - 1) // self.stride + 1
        big, small = (ka, ka, self.cin * s * s, self.cout), self.w_shape
        if (tuple(src.shape), tuple(dst.shape)) != ((big, small) if grad else (small, big)):
            raise _ffi.VltfError("conv.s2d_weights: shape mismatch %s -> %s" % (tuple(src.shape), tuple(dst.shape)))
        _ffi.call("vl_s2d_weights", self._d, _p(src), _p(dst), int(grad), stream())

    def c8_wgrad_ws_bytes(self, n):
        return int(_ffi.lib().vl_conv_c8_wgrad_ws_bytes(self._d, n))

    def c8_wgrad(self, xb, dyb, dw, ws):
        n = xb.shape[0]
        _f32(dw); _dense(dw, ws)
        self._c8_check(xb, n, self.cin, self.h, self.w, self.x_halo, "xb")
        self._c8_check(dyb, n, self.cout, self.oh, self.ow, self.dy_halo, "dyb")
        if tuple(dw.shape) != self.w_shape:
            raise _ffi.VltfError("conv.c8_wgrad: dw shape %s" % (tuple(dw.shape),))
        _ffi.call("vl_conv_c8_wgrad", self._d, _p(xb), _p(dyb), _p(dw), _p(ws), ws.numel() * ws.element_size(), n, stream())


def bias_grad_c8(dyb, db, ws, c, halo):
    """db[c] = sum over images and pixels of the packed gradient dyb (c8 with `halo`)."""
    _f32(db, ws); _dense(dyb, db, ws)
    n, cb, hp, wp, _ = dyb.shape
    if dyb.dtype != torch.bfloat16 or cb != (c + 7) // 8 or ws.numel() < 64 * 8 * cb:
        raise _ffi.VltfError("bias_grad_c8: dyb must be bf16 c8 of %d channels, ws >= 64 * 8 * blocks floats" % c)
    _ffi.call("vl_bias_grad_c8", _p(dyb), _p(db), _p(ws), n, c, hp - 2 * halo, wp - 2 * halo, halo, stream())


def kc8_shape(positions, channels):
    """Reduction-major packed operand of gemm_kc8: [ceil(channels / 8)][positions][8] bf16."""
    return ((channels + 7) // 8, positions, 8)


def pack_kc8(src, dst, positions, channels, pos_stride, ch_stride):
    """dst (kc8) = src[position * pos_stride + channel * ch_stride]: a row-major fp32 matrix (or its transpose, by the strides)."""
    _f32(src); _dense(dst)
    if dst.dtype != torch.bfloat16 or tuple(dst.shape) != kc8_shape(positions, channels):
        raise _ffi.VltfError("pack_kc8: dst must be bf16 %s, got %s %s" % (kc8_shape(positions, channels), dst.dtype, tuple(dst.shape)))
    if (positions - 1) * pos_stride + (channels - 1) * ch_stride >= src.numel():
        raise _ffi.VltfError("pack_kc8: strides reach past the source")
    _ffi.call("vl_pack_kc8", _p(src), _p(dst), positions, channels, pos_stride, ch_stride, stream())


def gemm_kc8_ws_bytes(m, n, k):
    return int(_ffi.lib().vl_gemm_kc8_ws_bytes(m, n, k))


def gemm_kc8(a, b, c, m, n, k, bias=None, relu=False, ws=None):
    """c[m][n] = sum_k a[k][m] b[k][n] (+bias) (relu): bf16 products of kc8 operands, fp32 accumulation and output."""
    _f32(c, bias); _dense(a, b, c, bias, ws)
    if a.dtype != torch.bfloat16 or b.dtype != torch.bfloat16 or tuple(a.shape) != kc8_shape(k, m) or tuple(b.shape) != kc8_shape(k, n) \
            or c.numel() < m * n:
        raise _ffi.VltfError("gemm_kc8: operand shapes a=%s b=%s for m=%d n=%d k=%d" % (tuple(a.shape), tuple(b.shape), m, n, k))
    _ffi.call("vl_gemm_kc8", _p(a), _p(b), _p(c), m, n, k, _p(bias), int(relu), _p(ws), 0 if ws is None else ws.numel() * ws.element_size(),
              stream())


def c8_shape(n, c, h, w, halo):
    return (n, (c + 7) // 8, h + 2 * halo, w + 2 * halo, 8)


def pack_c8(x, xb, x_halo, xb_halo):
    """fp32 NCHW (x_halo) -> bf16 c8 (xb_halo); xb zero-initialised once by the caller (only interiors are written)."""
    _f32(x); _dense(x, xb)
    n, c = x.shape[0], x.shape[1]
    h, w = x.shape[2] - 2 * x_halo, x.shape[3] - 2 * x_halo
    if xb.dtype != torch.bfloat16 or tuple(xb.shape) != c8_shape(n, c, h, w, xb_halo):
        raise _ffi.VltfError("pack_c8: xb must be bf16 %s, got %s %s" % (c8_shape(n, c, h, w, xb_halo), xb.dtype, tuple(xb.shape)))
    _ffi.call("vl_pack_c8", _p(x), _p(xb), n, c, h, w, x_halo, xb_halo, stream())


def bias_grad_nchw(dy, db, ws):
    _f32(dy, db, ws); _dense(dy, db, ws)
    n, c = dy.shape[0], dy.shape[1]
    hw = dy.numel() // (n * c)
    if ws.numel() < 64 * c:
        raise _ffi.VltfError("bias_grad_nchw: workspace needs 64*c floats")
    _ffi.call("vl_bias_grad_nchw", _p(dy), _p(db), _p(ws), n, c, hw, stream())


# ---- LRN / pool ----------------------------------------------------------------------------------
def lrn_fwd(x, y, radius=2, alpha=2e-5, beta=0.75, bias=1.0):
    _f32(x, y); _dense(x, y)
    n, c = x.shape[0], x.shape[1]
    _ffi.call("vl_lrn_fwd", _p(x), _p(y), n, c, x.numel() // (n * c), radius, alpha, beta, bias, stream())


def lrn_bwd(x, dy, dx, radius=2, alpha=2e-5, beta=0.75, bias=1.0, relu_fused=False, dx_halo=0):
    _f32(x, dy, dx); _dense(x, dy, dx)
    n, c, h, w = x.shape
    if tuple(dx.shape) != (n, c, h + 2 * dx_halo, w + 2 * dx_halo):
        raise _ffi.VltfError("lrn_bwd: dx shape %s does not match x %s with halo %d" % (tuple(dx.shape), tuple(x.shape), dx_halo))
    _ffi.call("vl_lrn_bwd", _p(x), _p(dy), _p(dx), n, c, h * w, radius, alpha, beta, bias, int(relu_fused), w, dx_halo, stream())


def pool_out(h, k=3, s=2):
    return (h - k) // s + 1


def _pool_layout(c, oh, ow, hwc, halo):
    """(element offset of the interior origin, strides n/c/h/w) of a pool output: NCHW with halo, or the
    (h, w, c)-flat order fc6 expects (alexnet.py:228)."""
    if hwc:
        return 0, (oh * ow * c, 1, ow * c, c)
    wp = ow + 2 * halo
    pp = (oh + 2 * halo) * wp
    return halo * wp + halo, (c * pp, pp, wp, 1)


def maxpool_fwd(x, y, argmax, k=3, s=2, hwc=False, y_halo=0):
    _f32(x, y); _dense(x, y, argmax)
    n, c, h, w = x.shape
    o, st = _pool_layout(c, pool_out(h, k, s), pool_out(w, k, s), hwc, y_halo)
    _ffi.call("vl_maxpool_fwd", _p(x), _p(y) + 4 * o, None if argmax is None else _p(argmax) + o, n, c, h, w, k, s, st[0], st[1],
              st[2], st[3], stream())


def maxpool_bwd(dy, argmax, dx, relu_mask=None, k=3, s=2, hwc=False, dy_halo=0, dx_halo=0):
    """dy / argmax have the pool OUTPUT layout (halo dy_halo); dx is NCHW with dx_halo."""
    _f32(dy, dx, relu_mask); _dense(dy, dx, argmax, relu_mask)
    n, c = dx.shape[0], dx.shape[1]
    h, w = dx.shape[2] - 2 * dx_halo, dx.shape[3] - 2 * dx_halo
    o, st = _pool_layout(c, pool_out(h, k, s), pool_out(w, k, s), hwc, dy_halo)
    _ffi.call("vl_maxpool_bwd", _p(dy) + 4 * o, _p(argmax) + o, _p(dx), _p(relu_mask), n, c, h, w, k, s, st[0], st[1], st[2], st[3],
              dx_halo, stream())


def lrn_pool_fwd(x, p, argmax, p_halo=0, radius=2, alpha=2e-5, beta=0.75, bias=1.0):
    """Fused LRN + maxpool(3,2) forward; p / argmax have the pool-output layout (p_halo); the LRN output is not stored."""
    _f32(x, p); _dense(x, p, argmax)
    n, c, h, w = x.shape
    want = (n, c, pool_out(h) + 2 * p_halo, pool_out(w) + 2 * p_halo)
    if tuple(p.shape) != want or tuple(argmax.shape) != want:
        raise _ffi.VltfError("lrn_pool_fwd: shape mismatch x=%s p=%s argmax=%s" % (tuple(x.shape), tuple(p.shape), tuple(argmax.shape)))
    _ffi.call("vl_lrn_pool_fwd", _p(x), _p(p), _p(argmax), n, c, h, w, p_halo, radius, alpha, beta, bias, stream())


def _x_or_packed(x, c):
    """(packed?, n, h, w) of a pool / LRN input: fp32 NCHW, or bf16 c8 without a halo ([n][c/8][h][w][8]) of c channels."""
    if x.dtype == torch.bfloat16:
        if x.dim() != 5 or x.shape[4] != 8 or c is None or x.shape[1] != (c + 7) // 8 or not x.is_contiguous():
            raise _ffi.VltfError("packed pool input must be a contiguous bf16 [n][c/8][h][w][8] tensor and needs channels=")
        return 1, x.shape[0], x.shape[2], x.shape[3]
    _f32(x)
    return 0, x.shape[0], x.shape[2], x.shape[3]


def lrn_pool_fwd_c8(x, pb, argmax, p_halo=0, radius=2, alpha=2e-5, beta=0.75, bias=1.0, channels=None):
    """lrn_pool_fwd with the pooled output written as packed bf16 (c8 layout, p_halo): the next conv's operand on the bf16 path.
    x: fp32 NCHW, or the packed conv output (bf16 c8, no halo; pass channels=)."""
    _dense(x, pb, argmax)
    c = channels if channels is not None else x.shape[1]
    packed, n, h, w = _x_or_packed(x, c)
    oh, ow = pool_out(h), pool_out(w)
    if pb.dtype != torch.bfloat16 or tuple(pb.shape) != c8_shape(n, c, oh, ow, p_halo) or \
            tuple(argmax.shape) != (n, c, oh + 2 * p_halo, ow + 2 * p_halo):
        raise _ffi.VltfError("lrn_pool_fwd_c8: shape mismatch x=%s pb=%s argmax=%s" % (tuple(x.shape), tuple(pb.shape), tuple(argmax.shape)))
    _ffi.call("vl_lrn_pool_fwd_c8", _p(x), packed, _p(pb), _p(argmax), n, c, h, w, p_halo, radius, alpha, beta, bias, stream())


def pool_lrn_bwd(x, dp, argmax, dx, p_halo=0, dx_halo=0, radius=2, alpha=2e-5, beta=0.75, bias=1.0, relu_fused=True):
    """Fused maxpool(3,2) backward + LRN backward (+ReluGrad); dp/argmax have the pool-output layout (p_halo)."""
    _f32(x, dp, dx); _dense(x, dp, argmax, dx)
    n, c, h, w = x.shape
    oh, ow = pool_out(h), pool_out(w)
    if tuple(dp.shape) != (n, c, oh + 2 * p_halo, ow + 2 * p_halo) or tuple(argmax.shape) != tuple(dp.shape) or \
            tuple(dx.shape) != (n, c, h + 2 * dx_halo, w + 2 * dx_halo):
        raise _ffi.VltfError("pool_lrn_bwd: shape mismatch x=%s dp=%s dx=%s" % (tuple(x.shape), tuple(dp.shape), tuple(dx.shape)))
    _ffi.call("vl_pool_lrn_bwd", _p(x), _p(dp), _p(argmax), _p(dx), n, c, h, w, p_halo, radius, alpha, beta, bias, int(relu_fused),
              dx_halo, stream())


def pool_lrn_bwd_test_ranges(ranges=0):
    """Test hook: force the channel-range count of pool_lrn_bwd / pool_lrn_bwd_c8 launches (1..4); 0 = the launcher's own choice."""
    _ffi.call("vl_pool_lrn_bwd_test_ranges", int(ranges))


def pool_lrn_bwd_c8(x, dp, argmax, dxb, p_halo=0, dxb_halo=0, radius=2, alpha=2e-5, beta=0.75, bias=1.0, relu_fused=True):
    """pool_lrn_bwd with the gradient written as packed bf16 (c8 layout, dxb_halo): the bf16 conv path's operand.
    x: fp32 NCHW, or the packed conv output (bf16 c8, no halo)."""
    _f32(dp); _dense(x, dp, argmax, dxb)
    c = dp.shape[1]
    packed, n, h, w = _x_or_packed(x, c)
    oh, ow = pool_out(h), pool_out(w)
    if tuple(dp.shape) != (n, c, oh + 2 * p_halo, ow + 2 * p_halo) or tuple(argmax.shape) != tuple(dp.shape) or \
            dxb.dtype != torch.bfloat16 or tuple(dxb.shape) != c8_shape(n, c, h, w, dxb_halo):
        raise _ffi.VltfError("pool_lrn_bwd_c8: shape mismatch x=%s dp=%s dxb=%s" % (tuple(x.shape), tuple(dp.shape), tuple(dxb.shape)))
    _ffi.call("vl_pool_lrn_bwd_c8", _p(x), packed, _p(dp), _p(argmax), _p(dxb), n, c, h, w, p_halo, radius, alpha, beta, bias, int(relu_fused),
              dxb_halo, stream())


# ---- dense ---------------------------------------------------------------------------------------
def gemm(a, b, c, m, n, k, transa=False, transb=False, lda=None, ldb=None, ldc=None, bias=None, relu=False,
         relu_mask=None, ws=None):
    """c[m,n] = op(a) @ op(b) (+bias) (relu) (mask).  a/b/c may be views: only data_ptr + ld are used."""
    _f32(a, b, c, bias, relu_mask)
    lda = lda if lda is not None else (m if transa else k)
    ldb = ldb if ldb is not None else (k if transb else n)
    ldc = ldc if ldc is not None else n
    nbytes = 0 if ws is None else ws.numel() * ws.element_size()
    _ffi.call("vl_gemm", int(transa), int(transb), m, n, k, _p(a), lda, _p(b), ldb, _p(c), ldc, _p(bias), int(relu),
              _p(relu_mask), _p(ws), nbytes, stream())


def gemm_split_ws_bytes(m, n, k):
    """Workspace with which gemm() runs in the split-bf16 arithmetic of set_conv_math (vl_gemm_split_ws_bytes)."""
    return int(_ffi.lib().vl_gemm_split_ws_bytes(int(m), int(n), int(k)))


def colsum(a, out, ws, m, n, lda=None):
    _f32(a, out, ws)
    if ws.numel() < 64 * n:
        raise _ffi.VltfError("colsum: workspace needs 64*n floats")
    _ffi.call("vl_colsum", _p(a), lda if lda is not None else n, _p(out), _p(ws), m, n, stream())


# ---- LSTM ----------------------------------------------------------------------------------------
def lstm_step_fwd(gx, gh, act, cseq, hseq, hprev, batch, T, t, H, forget_bias=1.0):
    _f32(gx, gh, act, cseq, hseq, hprev)
    _ffi.call("vl_lstm_step_fwd", _p(gx), _p(gh), _p(act), _p(cseq), _p(hseq), _p(hprev), batch, T, t, H, forget_bias,
              stream())


def lstm_step_bwd(dout, dh_next, act, cseq, dc, dz, batch, T, t, H):
    _f32(dout, dh_next, act, cseq, dc, dz)
    _ffi.call("vl_lstm_step_bwd", _p(dout), _p(dh_next), _p(act), _p(cseq), _p(dc), _p(dz), batch, T, t, H, stream())


def lstm_seq_ws(batch, T, H, device):
    """Scratch for lstm_seq_fwd / lstm_seq_bwd (vl_lstm_seq_ws_bytes): the exchange words of the cluster form."""
    n = int(_ffi.lib().vl_lstm_seq_ws_bytes(int(batch), int(T), int(H)))
    return torch.zeros((n + 3) // 4, dtype=torch.float32, device=device)


def _seq_len(seq_len, batch, what):
    """Per-clip lengths of the *_len entry points: int32, contiguous, on the device, at least `batch` entries."""
    if not (torch.is_tensor(seq_len) and seq_len.dtype == torch.int32 and seq_len.is_cuda and seq_len.is_contiguous()
            and seq_len.numel() >= batch):
        raise _ffi.VltfError("%s: seq_len must be a contiguous int32 device tensor of at least %d entries" % (what, batch))
    return seq_len


def lstm_seq_fwd(gx, kh, act, cseq, hseq, hprev, batch, T, H, forget_bias=1.0, ws=None, h0=None, c0=None, seq_len=None):
    """All T steps in one launch; kh = kernel[D:] view ([H, 4H]); h0 / c0: initial state [batch, H] (None = zeros).
    seq_len: int32 device tensor [batch] of per-clip lengths (vl_lstm_seq_fwd_len: dead steps carry the state and output zero)."""
    _f32(gx, kh, act, cseq, hseq, hprev, h0, c0, ws)
    if ws is None:
        raise _ffi.VltfError("lstm_seq_fwd: a workspace from lstm_seq_ws() is required")
    if seq_len is not None:
        _ffi.call("vl_lstm_seq_fwd_len", _p(gx), _p(kh), _p(h0), _p(c0), _p(act), _p(cseq), _p(hseq), _p(hprev), batch, T, H,
                  forget_bias, _p(_seq_len(seq_len, batch, "lstm_seq_fwd")), _p(ws), ws.numel() * 4, stream())
        return
    _ffi.call("vl_lstm_seq_fwd", _p(gx), _p(kh), _p(h0), _p(c0), _p(act), _p(cseq), _p(hseq), _p(hprev), batch, T, H, forget_bias,
              _p(ws), ws.numel() * 4, stream())


def lstm_seq_bwd(dout, kh, act, cseq, dz, batch, T, H, ws=None, c0=None, dh0=None, dc0=None, seq_len=None):
    """BPTT in one launch; kh = kernel[D:] view (not transposed); dh0 / dc0: optional outputs [batch, H].
    seq_len: the lengths given to the forward call (vl_lstm_seq_bwd_len: dead rows of dout are ignored, their dz is 0)."""
    _f32(dout, kh, act, cseq, dz, c0, dh0, dc0, ws)
    if ws is None:
        raise _ffi.VltfError("lstm_seq_bwd: a workspace from lstm_seq_ws() is required")
    if seq_len is not None:
        _ffi.call("vl_lstm_seq_bwd_len", _p(dout), _p(kh), _p(act), _p(cseq), _p(c0), _p(dz), _p(dh0), _p(dc0), batch, T, H,
                  _p(_seq_len(seq_len, batch, "lstm_seq_bwd")), _p(ws), ws.numel() * 4, stream())
        return
    _ffi.call("vl_lstm_seq_bwd", _p(dout), _p(kh), _p(act), _p(cseq), _p(c0), _p(dz), _p(dh0), _p(dc0), batch, T, H, _p(ws),
              ws.numel() * 4, stream())


def lstm_seq_tag_span(batch, T, H):
    """Exchange tags one lstm_seq_fwd_st / lstm_seq_bwd_st call uses above its tag offset (0: the per-clip form, no tags)."""
    return int(_ffi.lib().vl_lstm_seq_tag_span(int(batch), int(T), int(H)))


def lstm_seq_fwd_st(gx, kh, act, cseq, hseq, hprev, batch, T, H, forget_bias=1.0, ws=None, state=None, tag_offset=0, h0=None, c0=None):
    """lstm_seq_fwd with replay-safe tags: base = state's tag origin (read on the device) + tag_offset (vl_lstm_seq_fwd_st)."""
    _f32(gx, kh, act, cseq, hseq, hprev, h0, c0, ws)
    if ws is None or state is None:
        raise _ffi.VltfError("lstm_seq_fwd_st: a workspace from lstm_seq_ws() and a step state are required")
    _ffi.call("vl_lstm_seq_fwd_st", _p(gx), _p(kh), _p(h0), _p(c0), _p(act), _p(cseq), _p(hseq), _p(hprev), batch, T, H, forget_bias,
              _p(ws), ws.numel() * 4, _state(state), int(tag_offset), stream())


def lstm_seq_bwd_st(dout, kh, act, cseq, dz, batch, T, H, ws=None, state=None, tag_offset=0, c0=None, dh0=None, dc0=None):
    _f32(dout, kh, act, cseq, dz, c0, dh0, dc0, ws)
    if ws is None or state is None:
        raise _ffi.VltfError("lstm_seq_bwd_st: a workspace from lstm_seq_ws() and a step state are required")
    _ffi.call("vl_lstm_seq_bwd_st", _p(dout), _p(kh), _p(act), _p(cseq), _p(c0), _p(dz), _p(dh0), _p(dc0), batch, T, H, _p(ws),
              ws.numel() * 4, _state(state), int(tag_offset), stream())


def _pair(v, what):
    """A (forward, backward) pair of the bidirectional entry points; None = (None, None)."""
    if v is None:
        return (None, None)
    if not (isinstance(v, (tuple, list)) and len(v) == 2):
        raise _ffi.VltfError("%s: expected a (forward, backward) pair of tensors" % what)
    return tuple(v)


def _row_stride(pair, H, ld, what):
    """Row stride (floats) of a strided pair (hseq / dout): `ld`, or H for two dense tensors."""
    ld = int(H if ld is None else ld)
    for t in pair:
        if t is not None and ld == H and not t.is_contiguous():
            raise _ffi.VltfError("%s: a view into a wider tensor needs its row stride (ld)" % what)
    return ld


def lstm_seq_bi_fwd(gx, kh, act, cseq, hseq, hprev, batch, T, H, forget_bias=1.0, ws=None, h0=None, c0=None, seq_len=None,
                    hseq_ld=None, state=None, tag_offset=0):
    """Both directions of a bidirectional layer in one launch (vl_lstm_seq_bi_fwd).  gx, kh, act, cseq, hseq, hprev, h0, c0 are
    (forward, backward) pairs; the backward cell runs over the reversed live prefix and stores by time index.  hseq_ld: row stride
    of both hseq tensors (2 H with hseq = (out[:, :H], out[:, H:]) of one [batch T, 2H] tensor).  state: a step state -> the
    replay-safe form (vl_lstm_seq_bi_fwd_st: no lengths), its tags from tag_offset."""
    what = "lstm_seq_bi_fwd"
    gx, kh, act, cseq, hseq, hprev, h0, c0 = (_pair(v, what) for v in (gx, kh, act, cseq, hseq, hprev, h0, c0))
    _f32(*gx, *kh, *act, *cseq, *hseq, *hprev, *h0, *c0, ws)
    _dense(*gx, *kh, *act, *cseq, *hprev, *h0, *c0)
    if ws is None:
        raise _ffi.VltfError("lstm_seq_bi_fwd: a workspace from lstm_seq_ws() is required")
    ptrs = [_p(t) for pr in (gx, kh, h0, c0, act, cseq, hseq) for t in pr] + [_row_stride(hseq, H, hseq_ld, what), _p(hprev[0]), _p(hprev[1])]
    if state is not None:
        if seq_len is not None:
            raise _ffi.VltfError("lstm_seq_bi_fwd: the replay-safe form takes no lengths")
        _ffi.call("vl_lstm_seq_bi_fwd_st", *ptrs, batch, T, H, forget_bias, _p(ws), ws.numel() * 4, _state(state), int(tag_offset), stream())
        return
    _ffi.call("vl_lstm_seq_bi_fwd", *ptrs, batch, T, H, forget_bias, _p(None if seq_len is None else _seq_len(seq_len, batch, what)),
              _p(ws), ws.numel() * 4, stream())


def lstm_seq_bi_bwd(dout, kh, act, cseq, dz, batch, T, H, ws=None, c0=None, dh0=None, dc0=None, seq_len=None, dout_ld=None, state=None,
                    tag_offset=0):
    """BPTT of both directions in one launch (vl_lstm_seq_bi_bwd); pairs as in lstm_seq_bi_fwd, dout (nullable, each half too) with row
    stride dout_ld; dh0 / dc0: optional output pairs.  state: the replay-safe form (vl_lstm_seq_bi_bwd_st)."""
    what = "lstm_seq_bi_bwd"
    dout, kh, act, cseq, dz, c0, dh0, dc0 = (_pair(v, what) for v in (dout, kh, act, cseq, dz, c0, dh0, dc0))
    _f32(*dout, *kh, *act, *cseq, *dz, *c0, *dh0, *dc0, ws)
    _dense(*kh, *act, *cseq, *dz, *c0, *dh0, *dc0)
    if ws is None:
        raise _ffi.VltfError("lstm_seq_bi_bwd: a workspace from lstm_seq_ws() is required")
    ptrs = [_p(dout[0]), _p(dout[1]), _row_stride(dout, H, dout_ld, what)] + [_p(t) for pr in (kh, act, cseq, c0, dz, dh0, dc0) for t in pr]
    if state is not None:
        if seq_len is not None:
            raise _ffi.VltfError("lstm_seq_bi_bwd: the replay-safe form takes no lengths")
        _ffi.call("vl_lstm_seq_bi_bwd_st", *ptrs, batch, T, H, _p(ws), ws.numel() * 4, _state(state), int(tag_offset), stream())
        return
    _ffi.call("vl_lstm_seq_bi_bwd", *ptrs, batch, T, H, _p(None if seq_len is None else _seq_len(seq_len, batch, what)), _p(ws),
              ws.numel() * 4, stream())


def lstm_seq_bi_tag_span(batch, T, H):
    """Exchange tags one replay-safe bidirectional call uses above its tag offset (0: H or the device cannot take the launch)."""
    return int(_ffi.lib().vl_lstm_seq_bi_tag_span(int(batch), int(T), int(H)))


GRU_MAX_HIDDEN = 512        # the GRU recurrence exists in the cluster form only (vltf.h: vl_gru_seq_fwd)


def gru_seq_fwd(gx, rk, act, hcand, hseq, hprev, batch, T, H, ws=None, rb=None, h0=None, seq_len=None, state=None, tag_offset=0):
    """The reset-after GRU recurrence, all T steps in one launch (vl_gru_seq_fwd).  gx [batch T, 3H]: input projections (z | r | n);
    rk = recurrent_kernel [H, 3H]; rb = recurrent_bias [3H] (None = zeros); h0 [batch, H] (None = zeros).  Writes act (activated z, r,
    n), hcand (the candidate's recurrent term), hseq, hprev.  ws: a workspace from lstm_seq_ws().  seq_len: int32 device tensor [batch]
    (dead steps carry h and write zeros).  state: a step state -> the replay-safe form (vl_gru_seq_fwd_st: no lengths), tags from
    tag_offset."""
    _f32(gx, rk, act, hcand, hseq, hprev, rb, h0, ws)
    _dense(gx, rk, act, hcand, hseq, hprev, rb, h0)
    if ws is None:
        raise _ffi.VltfError("gru_seq_fwd: a workspace from lstm_seq_ws() is required")
    ptrs = [_p(t) for t in (gx, rk, rb, h0, act, hcand, hseq, hprev)]
    if state is not None:
        if seq_len is not None:
            raise _ffi.VltfError("gru_seq_fwd: the replay-safe form takes no lengths")
        _ffi.call("vl_gru_seq_fwd_st", *ptrs, batch, T, H, _p(ws), ws.numel() * 4, _state(state), int(tag_offset), stream())
        return
    _ffi.call("vl_gru_seq_fwd", *ptrs, batch, T, H, _p(None if seq_len is None else _seq_len(seq_len, batch, "gru_seq_fwd")), _p(ws),
              ws.numel() * 4, stream())


def gru_seq_bwd(dout, rk, act, hcand, hprev, dgx, dgh, batch, T, H, ws=None, dh0=None, seq_len=None, state=None, tag_offset=0):
    """BPTT of gru_seq_fwd in one launch (vl_gru_seq_bwd): reads dout (None = zeros) and the forward's act, hcand, hprev; writes dgx and dgh
    [batch T, 3H] (the gradients of the two pre-activation terms) and, when given, dh0 [batch, H].  seq_len / state as in gru_seq_fwd."""
    _f32(dout, rk, act, hcand, hprev, dgx, dgh, dh0, ws)
    _dense(dout, rk, act, hcand, hprev, dgx, dgh, dh0)
    if ws is None:
        raise _ffi.VltfError("gru_seq_bwd: a workspace from lstm_seq_ws() is required")
    ptrs = [_p(t) for t in (dout, rk, act, hcand, hprev, dgx, dgh, dh0)]
    if state is not None:
        if seq_len is not None:
            raise _ffi.VltfError("gru_seq_bwd: the replay-safe form takes no lengths")
        _ffi.call("vl_gru_seq_bwd_st", *ptrs, batch, T, H, _p(ws), ws.numel() * 4, _state(state), int(tag_offset), stream())
        return
    _ffi.call("vl_gru_seq_bwd", *ptrs, batch, T, H, _p(None if seq_len is None else _seq_len(seq_len, batch, "gru_seq_bwd")), _p(ws),
              ws.numel() * 4, stream())


def gru_seq_tag_span(batch, T, H):
    """Exchange tags one replay-safe gru_seq_fwd / gru_seq_bwd call uses above its tag offset (0: H is refused)."""
    return int(_ffi.lib().vl_gru_seq_tag_span(int(batch), int(T), int(H)))


def lstm_seq_ws_clear(ws):
    """Zeroes the exchange words of a workspace (not its time-out word), on the stream: its owner restarts its tags."""
    _f32(ws)
    _ffi.call("vl_lstm_seq_ws_clear", _p(ws), ws.numel() * 4, stream())


def lstm_seq_timed_out(ws):
    """True if a workgroup of any cluster-form launch on `ws` since the last call gave up waiting for its peers; the flag is
    sticky across launches and reset by this read (synchronises)."""
    v = C.c_int(0)
    _ffi.call("vl_lstm_seq_status", _p(ws), C.byref(v))
    return bool(v.value)


def lstm_seq_check(*workspaces):
    """Raises VltfError when a cluster-form LSTM launch on one of the workspaces timed out (results of that step are invalid)."""
    bad = [i for i, ws in enumerate(workspaces) if ws is not None and lstm_seq_timed_out(ws)]
    if bad:
        raise _ffi.VltfError("LSTM cluster kernel timed out waiting for its peer workgroups (workspace %s): the recurrence needs "
                             "every workgroup resident at once and another kernel was holding compute units; this step's results "
                             "are invalid" % bad)


def lstm_seq_test_hooks(spin_limit=0, mute_workgroup=-1):
    """Test hooks (vl_lstm_seq_test_hooks): shorter spin limit / one workgroup that never publishes.  Defaults restore production."""
    _ffi.call("vl_lstm_seq_test_hooks", int(spin_limit), int(mute_workgroup))


def transpose(src, dst, rows, cols, ld=None):
    _f32(src, dst)
    _ffi.call("vl_transpose", _p(src), ld if ld is not None else cols, _p(dst), rows, cols, stream())


FUSION_CODE = {"avg": 0, "last": 1}


def temporal_fusion_fwd(x, y, batch, T, H, method, seq_len=None):
    """seq_len: int32 device tensor [batch]; clip b fuses its first seq_len[b] steps (last = step len - 1, avg = sum / len)."""
    _f32(x, y)
    if seq_len is not None:
        _ffi.call("vl_temporal_fusion_fwd_len", _p(x), _p(y), batch, T, H, FUSION_CODE[method],
                  _p(_seq_len(seq_len, batch, "temporal_fusion_fwd")), stream())
        return
    _ffi.call("vl_temporal_fusion_fwd", _p(x), _p(y), batch, T, H, FUSION_CODE[method], stream())


def temporal_fusion_bwd(dy, dx, batch, T, H, method, seq_len=None):
    _f32(dy, dx)
    if seq_len is not None:
        _ffi.call("vl_temporal_fusion_bwd_len", _p(dy), _p(dx), batch, T, H, FUSION_CODE[method],
                  _p(_seq_len(seq_len, batch, "temporal_fusion_bwd")), stream())
        return
    _ffi.call("vl_temporal_fusion_bwd", _p(dy), _p(dx), batch, T, H, FUSION_CODE[method], stream())


ATTN_MAX_T = 1024       # vl_attn_pool_*: a clip's scores live in LDS


def _attn_sizes(who, batch, T, HO, A, **tensors):
    """Every tensor given holds at least what the launch reads or writes of it (None passes: the C side refuses a null pointer)."""
    need = dict(u=batch * T * A, s=batch * T * A, du=batch * T * A, h=batch * T * HO, dh=batch * T * HO, alpha=batch * T,
                y=batch * HO, dy=batch * HO, dcp=batch * A, c=A)
    for k, t in tensors.items():
        if t is not None and min(batch, T, HO, A) > 0 and t.numel() < need[k]:
            raise _ffi.VltfError("%s: %s has %d elements, the launch needs %d" % (who, k, t.numel(), need[k]))


def attn_pool_fwd(u, c, h, s, alpha, y, batch, T, HO, A, seq_len=None):
    """Attention pooling over time (vl_attn_pool_fwd): s = tanh(u) (s may be u), alpha = softmax over the live steps of s . c,
    y = sum_t alpha_t h_t.  u, s [batch, T, A]; c [A]; h [batch, T, HO]; alpha [batch, T]; y [batch, HO]; seq_len as temporal_fusion_fwd."""
    _f32(u, c, h, s, alpha, y)
    _dense(u, c, h, s, alpha, y)
    _attn_sizes("attn_pool_fwd", batch, T, HO, A, u=u, c=c, h=h, s=s, alpha=alpha, y=y)
    _ffi.call("vl_attn_pool_fwd", _p(u), _p(c), _p(h), None if seq_len is None else _p(_seq_len(seq_len, batch, "attn_pool_fwd")),
              _p(s), _p(alpha), _p(y), batch, T, HO, A, stream())


def attn_pool_bwd(dy, h, s, alpha, c, du, dh, dcp, batch, T, HO, A, seq_len=None):
    """Its backward (vl_attn_pool_bwd): du [batch, T, A], the direct term dh [batch, T, HO] = alpha_t dy and the per-clip partials
    dcp [batch, A] of c's gradient; dead rows of du and dh are zeros."""
    _f32(dy, h, s, alpha, c, du, dh, dcp)
    _dense(dy, h, s, alpha, c, du, dh, dcp)
    _attn_sizes("attn_pool_bwd", batch, T, HO, A, dy=dy, h=h, s=s, alpha=alpha, c=c, du=du, dh=dh, dcp=dcp)
    _ffi.call("vl_attn_pool_bwd", _p(dy), _p(h), _p(s), _p(alpha), _p(c),
              None if seq_len is None else _p(_seq_len(seq_len, batch, "attn_pool_bwd")), _p(du), _p(dh), _p(dcp), batch, T, HO, A,
              stream())


MHSA_MAX_T, MHSA_MAX_HIDDEN, MHSA_MIN_HEAD, MHSA_MAX_HEAD = 64, 1024, 8, 128       # vl_mhsa_*: vltf.h


def _mhsa_sizes(who, batch, T, H, heads, **tensors):
    """The limits of vl_mhsa_* (the C side's wording), then every tensor given holds at least what the launch reads or writes of it
    (None passes: the C side refuses a null pointer it needs).  Raises before any launch."""
    if min(batch, T, H, heads) <= 0:
        raise _ffi.VltfError("%s: batch %d, T %d, H %d, heads %d must be positive" % (who, batch, T, H, heads))
    if T > MHSA_MAX_T:
        raise _ffi.VltfError("%s: T %d exceeds %d (a head's score tile lives in LDS, a key per lane)" % (who, T, MHSA_MAX_T))
    if H > MHSA_MAX_HIDDEN:
        raise _ffi.VltfError("%s: H %d exceeds %d" % (who, H, MHSA_MAX_HIDDEN))
    if H % heads:
        raise _ffi.VltfError("%s: heads %d does not divide H %d" % (who, heads, H))
    if not MHSA_MIN_HEAD <= H // heads <= MHSA_MAX_HEAD:
        raise _ffi.VltfError("%s: the head width H / heads = %d must lie in %d..%d" % (who, H // heads, MHSA_MIN_HEAD, MHSA_MAX_HEAD))
    rows = batch * T
    need = dict(qkv=rows * 3 * H, dqkv=rows * 3 * H, ctx=rows * H, dctx=rows * H, P=batch * heads * T * T, pos=heads * (2 * T - 1),
                dposp=batch * heads * (2 * T - 1))
    for k, t in tensors.items():
        if t is not None and t.numel() < need[k]:
            raise _ffi.VltfError("%s: %s has %d elements, the launch needs %d" % (who, k, t.numel(), need[k]))


def mhsa_fwd(qkv, pos, P, ctx, batch, T, H, heads, seq_len=None):
    """Multi-head self-attention over time (vl_mhsa_fwd): per clip and head, P = softmax over the live keys of Q K^T / sqrt(H / heads) +
    pos[h, k - q + T - 1], ctx = P V.  qkv [batch T, 3H] (Q | K | V); pos [heads, 2T - 1] or None; P [batch, heads, T, T];
    ctx [batch T, H]; seq_len as gru_seq_fwd (dead rows of qkv are never read, dead rows / columns of P and dead rows of ctx are zeros)."""
    _f32(qkv, pos, P, ctx)
    _dense(qkv, pos, P, ctx)
    _mhsa_sizes("mhsa_fwd", batch, T, H, heads, qkv=qkv, pos=pos, P=P, ctx=ctx)
    _ffi.call("vl_mhsa_fwd", _p(qkv), _p(pos), None if seq_len is None else _p(_seq_len(seq_len, batch, "mhsa_fwd")), _p(P), _p(ctx),
              batch, T, H, heads, stream())


def mhsa_bwd(dctx, qkv, P, dqkv, dposp, batch, T, H, heads, seq_len=None):
    """Its backward (vl_mhsa_bwd): dqkv [batch T, 3H] (dead rows zeros) and, unless None, the per-clip partials dposp
    [batch, heads, 2T - 1] of pos's gradient (colsum them over the batch rows)."""
    _f32(dctx, qkv, P, dqkv, dposp)
    _dense(dctx, qkv, P, dqkv, dposp)
    _mhsa_sizes("mhsa_bwd", batch, T, H, heads, dctx=dctx, qkv=qkv, P=P, dqkv=dqkv, dposp=dposp)
    _ffi.call("vl_mhsa_bwd", _p(dctx), _p(qkv), _p(P), None if seq_len is None else _p(_seq_len(seq_len, batch, "mhsa_bwd")), _p(dqkv),
              _p(dposp), batch, T, H, heads, stream())


def live_rows(x, y, batch, T, W, seq_len):
    """y = x in the live rows of x [batch T, W], zeros in the dead ones (vl_live_rows)."""
    _f32(x, y)
    _dense(x, y)
    if min(batch, T, W) > 0 and min(x.numel(), y.numel()) < batch * T * W:
        raise _ffi.VltfError("live_rows: x / y hold %d / %d elements, the launch needs %d" % (x.numel(), y.numel(), batch * T * W))
    _ffi.call("vl_live_rows", _p(x), _p(_seq_len(seq_len, batch, "live_rows")), _p(y), batch, T, W, stream())


TCONV_MAX_TAPS, TCONV_MAX_DILATION, TCONV_MAX_WIDTH = 9, 65536, 1024                 # vl_tconv_cols_*: vltf.h


def _tconv_sizes(who, batch, T, C, taps, dilation, causal, **tensors):
    """The limits of vl_tconv_cols_* (the C side's wording), then every tensor given holds at least what the launch reads or writes of
    it (None passes: the C side refuses a null pointer it needs).  Raises before any launch."""
    if min(batch, T, C) <= 0:
        raise _ffi.VltfError("%s: batch %d, T %d, C %d must be positive" % (who, batch, T, C))
    if not 1 <= taps <= TCONV_MAX_TAPS:
        raise _ffi.VltfError("%s: taps %d must lie in 1..%d" % (who, taps, TCONV_MAX_TAPS))
    if not causal and taps % 2 == 0:
        raise _ffi.VltfError("%s: taps %d must be odd unless causal (a centred kernel has a middle tap)" % (who, taps))
    if not 1 <= dilation <= TCONV_MAX_DILATION:
        raise _ffi.VltfError("%s: dilation %d must lie in 1..%d" % (who, dilation, TCONV_MAX_DILATION))
    if C > TCONV_MAX_WIDTH:
        raise _ffi.VltfError("%s: C %d exceeds %d" % (who, C, TCONV_MAX_WIDTH))
    rows = batch * T
    need = dict(x=rows * C, dx=rows * C, dres=rows * C, cols=rows * taps * C, dcols=rows * taps * C)
    for k, t in tensors.items():
        if t is not None and t.numel() < need[k]:
            raise _ffi.VltfError("%s: %s has %d elements, the launch needs %d" % (who, k, t.numel(), need[k]))


def tconv_cols_fwd(x, cols, batch, T, C, taps, dilation=1, causal=False, seq_len=None):
    """The taps of a dilated convolution over time as the operand of a product (vl_tconv_cols_fwd): cols[b T + t, j C + c] =
    x[b T + t + off_j, c] inside the clip's live steps, +0.0 elsewhere; off_j = (j - (taps - 1) // 2) dilation, causal:
    (j - (taps - 1)) dilation.  x [batch T, C]; cols [batch T, taps C], every element written; seq_len as mhsa_fwd (dead rows of x
    are never read)."""
    _f32(x, cols)
    _dense(x, cols)
    _tconv_sizes("tconv_cols_fwd", batch, T, C, taps, dilation, causal, x=x, cols=cols)
    _ffi.call("vl_tconv_cols_fwd", _p(x), None if seq_len is None else _p(_seq_len(seq_len, batch, "tconv_cols_fwd")), _p(cols),
              batch, T, C, taps, dilation, int(bool(causal)), stream())


def tconv_cols_bwd(dcols, dres, dx, batch, T, C, taps, dilation=1, causal=False, seq_len=None):
    """Its backward (vl_tconv_cols_bwd): dx[b T + t, c] = dres[b T + t, c] + the sum over the taps j ascending of
    dcols[b T + t - off_j, j C + c] inside the live steps; dres (the gradient of a residual path) may be None; dead rows of dx are
    +0.0 and dead rows of dcols / dres are never read."""
    _f32(dcols, dres, dx)
    _dense(dcols, dres, dx)
    _tconv_sizes("tconv_cols_bwd", batch, T, C, taps, dilation, causal, dcols=dcols, dres=dres, dx=dx)
    _ffi.call("vl_tconv_cols_bwd", _p(dcols), _p(dres), None if seq_len is None else _p(_seq_len(seq_len, batch, "tconv_cols_bwd")),
              _p(dx), batch, T, C, taps, dilation, int(bool(causal)), stream())


LN_MIN_WIDTH, LN_MAX_WIDTH, LN_EPS = 8, 1024, 1e-5                               # vl_add_layer_norm_fwd / vl_layer_norm_bwd: vltf.h


def _ln_sizes(who, clips, T, W, **tensors):
    """The limits of the layer-norm launches (the C side's wording), then every tensor given holds at least what the launch reads or
    writes of it (None passes: the C side refuses a null pointer it needs).  Raises before any launch."""
    if min(clips, T) <= 0:
        raise _ffi.VltfError("%s: clips %d, T %d must be positive" % (who, clips, T))
    if not LN_MIN_WIDTH <= W <= LN_MAX_WIDTH:
        raise _ffi.VltfError("%s: the row width W %d must lie in %d..%d (a row lives in one wave's registers)"
                             % (who, W, LN_MIN_WIDTH, LN_MAX_WIDTH))
    rows = clips * T
    need = dict(gamma=W, beta=W, stats=2 * rows, dgb_partial=2 * clips * W)
    for k, t in tensors.items():
        if t is not None and t.numel() < need.get(k, rows * W):
            raise _ffi.VltfError("%s: %s has %d elements, the launch needs %d" % (who, k, t.numel(), need.get(k, rows * W)))


def add_layer_norm_fwd(x, r, sum, y, gamma, beta, stats, clips, T, W, eps=LN_EPS, seq_len=None):
    """A layer norm over the last axis with the residual add in front of it fused (vl_add_layer_norm_fwd): s = x + r (r None: s = x),
    stored to `sum` unless None; y = (s - mean) rstd gamma + beta; stats [clips T, 2] = mean, rstd for layer_norm_bwd.  Rows
    [clips T, W], 8 <= W <= 1024; seq_len as mhsa_fwd: dead rows of x and r are never read, dead rows of y, sum and stats are zeros."""
    _f32(x, r, sum, y, gamma, beta, stats)
    _dense(x, r, sum, y, gamma, beta, stats)
    _ln_sizes("add_layer_norm_fwd", clips, T, W, x=x, r=r, sum=sum, y=y, gamma=gamma, beta=beta, stats=stats)
    if not (eps > 0 and math.isfinite(eps)):
        raise _ffi.VltfError("add_layer_norm_fwd: eps %g must be positive and finite" % eps)
    _ffi.call("vl_add_layer_norm_fwd", _p(x), _p(r), _p(sum), _p(y), _p(gamma), _p(beta), _p(stats), clips, T, W, eps,
              None if seq_len is None else _p(_seq_len(seq_len, clips, "add_layer_norm_fwd")), stream())


def layer_norm_bwd(dy, s, gamma, stats, dres, dx, dgb_partial, clips, T, W, seq_len=None):
    """Its backward (vl_layer_norm_bwd) from the forward's s (`sum`, or x where there was no r) and stats: dx = rstd (dy^ - mean(dy^) -
    x^ mean(dy^ x^)) + dres with dy^ = dy gamma (dres None: no such term), dead rows zeros, and the per-clip partials dgb_partial
    [clips, 2W] of gamma's (columns 0 .. W) and beta's (W .. 2W) gradients over the clip's live rows (colsum them over the clips)."""
    _f32(dy, s, gamma, stats, dres, dx, dgb_partial)
    _dense(dy, s, gamma, stats, dres, dx, dgb_partial)
    _ln_sizes("layer_norm_bwd", clips, T, W, dy=dy, s=s, gamma=gamma, stats=stats, dres=dres, dx=dx, dgb_partial=dgb_partial)
    _ffi.call("vl_layer_norm_bwd", _p(dy), _p(s), _p(gamma), _p(stats), _p(dres), _p(dx), _p(dgb_partial), clips, T, W,
              None if seq_len is None else _p(_seq_len(seq_len, clips, "layer_norm_bwd")), stream())


def _gelu_sizes(who, count, **tensors):
    if count <= 0:
        raise _ffi.VltfError("%s: count %d must be positive" % (who, count))
    for k, t in tensors.items():
        if t is not None and t.numel() < count:
            raise _ffi.VltfError("%s: %s has %d elements, the launch needs %d" % (who, k, t.numel(), count))


def gelu_fwd(u, f, count):
    """f = gelu(u) over the first `count` elements, the exact (erf) form of Keras / torch (vl_gelu_fwd)."""
    _f32(u, f)
    _dense(u, f)
    _gelu_sizes("gelu_fwd", count, u=u, f=f)
    _ffi.call("vl_gelu_fwd", _p(u), _p(f), count, stream())


def gelu_bwd(df, u, du, count):
    """du = df gelu'(u) (vl_gelu_bwd); du may be df."""
    _f32(df, u, du)
    _dense(df, u, du)
    _gelu_sizes("gelu_bwd", count, df=df, u=u, du=du)
    _ffi.call("vl_gelu_bwd", _p(df), _p(u), _p(du), count, stream())


# ---- dropout of the self-attention model (vltf.h: vl_mhsa_drop_fwd ...) ---------------------------------------------------
SA_DROP_STREAM = 0x5AD000000000      # the stream constant of these launches' draws (csrc/common.h)
SA_DROP_SITES = ("weights", "attn_branch", "ffn_branch", "path")


def sa_drop_salt(node, layer, site):
    """The salt of one (node, layer, site) stream: node << 12 | layer << 2 | site (site: an entry of SA_DROP_SITES)."""
    layer, node = int(layer), int(node)
    if not (0 <= layer < 1024 and 0 <= node < (1 << 20)):
        raise _ffi.VltfError("sa_drop_salt: layer %d must lie in 0..1023 and node %d in 0..2^20 - 1" % (layer, node))
    return (node << 12) | (layer << 2) | SA_DROP_SITES.index(site)


def _sa_keep(who, **keeps):
    for k, v in keeps.items():
        if not (isinstance(v, (int, float, np.floating)) and not isinstance(v, bool) and 0.0 < float(v) <= 1.0):
            raise _ffi.VltfError("%s: %s %s must lie in (0, 1]" % (who, k, v))


def _sa_seed(who, seed, state, clip0, clips):
    """-> (suffix of the symbol, the seed argument): exactly one of seed / state; clip0 inside the range the launches take."""
    if (seed is None) == (state is None):
        raise _ffi.VltfError("%s: give the seed or the step state, one of the two" % who)
    if not 0 <= int(clip0) < (1 << 31) - max(int(clips), 0):
        raise _ffi.VltfError("%s: clip0 %d must lie in 0 .. 2^31 - clips" % (who, clip0))
    return ("", int(seed) & 0xFFFFFFFFFFFFFFFF) if state is None else ("_st", _state(state))


def mhsa_drop_fwd(qkv, pos, P, ctx, batch, T, H, heads, keep, salt, clip0=0, seed=None, state=None, seq_len=None):
    """mhsa_fwd with dropout on the weights (vl_mhsa_drop_fwd / _st): ctx = (P o M / keep) V, P stored undropped; element (b, h, q, k)
    draws from (seed, salt) at the counter (((clip0 + b) heads + h) T + q) T + k.  seed, or state: the step state it is formed from."""
    _f32(qkv, pos, P, ctx)
    _dense(qkv, pos, P, ctx)
    _mhsa_sizes("mhsa_drop_fwd", batch, T, H, heads, qkv=qkv, pos=pos, P=P, ctx=ctx)
    _sa_keep("mhsa_drop_fwd", keep=keep)
    sfx, sd = _sa_seed("mhsa_drop_fwd", seed, state, clip0, batch)
    _ffi.call("vl_mhsa_drop_fwd" + sfx, _p(qkv), _p(pos), None if seq_len is None else _p(_seq_len(seq_len, batch, "mhsa_drop_fwd")),
              _p(P), _p(ctx), batch, T, H, heads, keep, sd, int(salt), int(clip0), stream())


def mhsa_drop_bwd(dctx, qkv, P, dqkv, dposp, batch, T, H, heads, keep, salt, clip0=0, seed=None, state=None, seq_len=None):
    """Its backward (vl_mhsa_drop_bwd / _st): the mask is drawn again from the same counters; P is the undropped one the forward stored."""
    _f32(dctx, qkv, P, dqkv, dposp)
    _dense(dctx, qkv, P, dqkv, dposp)
    _mhsa_sizes("mhsa_drop_bwd", batch, T, H, heads, dctx=dctx, qkv=qkv, P=P, dqkv=dqkv, dposp=dposp)
    _sa_keep("mhsa_drop_bwd", keep=keep)
    sfx, sd = _sa_seed("mhsa_drop_bwd", seed, state, clip0, batch)
    _ffi.call("vl_mhsa_drop_bwd" + sfx, _p(dctx), _p(qkv), _p(P), None if seq_len is None else _p(_seq_len(seq_len, batch, "mhsa_drop_bwd")),
              _p(dqkv), _p(dposp), batch, T, H, heads, keep, sd, int(salt), int(clip0), stream())


def add_layer_norm_drop_fwd(x, r, sum, y, gamma, beta, stats, clips, T, W, keep, keep_path, salt_elem, salt_path, branch, clip0=0,
                            seed=None, state=None, eps=LN_EPS, seq_len=None):
    """add_layer_norm_fwd with the branch r dropped (vl_add_layer_norm_drop_fwd / _st): s = x + r f, f = (kept_e / keep) (path_kept /
    keep_path); element (b, t, col) draws at ((clip0 + b) T + t) W + col of the salt_elem stream, the clip's path at 2 (clip0 + b) +
    branch of the salt_path stream.  Either keep may be 1; `sum` receives the dropped sum."""
    _f32(x, r, sum, y, gamma, beta, stats)
    _dense(x, r, sum, y, gamma, beta, stats)
    _ln_sizes("add_layer_norm_drop_fwd", clips, T, W, x=x, r=r, sum=sum, y=y, gamma=gamma, beta=beta, stats=stats)
    if not (eps > 0 and math.isfinite(eps)):
        raise _ffi.VltfError("add_layer_norm_drop_fwd: eps %g must be positive and finite" % eps)
    _sa_keep("add_layer_norm_drop_fwd", keep=keep, keep_path=keep_path)
    sfx, sd = _sa_seed("add_layer_norm_drop_fwd", seed, state, clip0, clips)
    _ffi.call("vl_add_layer_norm_drop_fwd" + sfx, _p(x), _p(r), _p(sum), _p(y), _p(gamma), _p(beta), _p(stats), clips, T, W, eps,
              None if seq_len is None else _p(_seq_len(seq_len, clips, "add_layer_norm_drop_fwd")), keep, keep_path, sd, int(salt_elem),
              int(salt_path), int(branch), int(clip0), stream())


def branch_drop_grad(ds, dr, clips, T, W, keep, keep_path, salt_elem, salt_path, branch, clip0=0, seed=None, state=None, seq_len=None):
    """dr = ds f: the gradient that enters a branch add_layer_norm_drop_fwd dropped, f drawn again (vl_branch_drop_grad / _st); dead
    rows zeros."""
    _f32(ds, dr)
    _dense(ds, dr)
    _ln_sizes("branch_drop_grad", clips, T, W, ds=ds, dr=dr)
    _sa_keep("branch_drop_grad", keep=keep, keep_path=keep_path)
    sfx, sd = _sa_seed("branch_drop_grad", seed, state, clip0, clips)
    _ffi.call("vl_branch_drop_grad" + sfx, _p(ds), _p(dr), clips, T, W,
              None if seq_len is None else _p(_seq_len(seq_len, clips, "branch_drop_grad")), keep, keep_path, sd, int(salt_elem),
              int(salt_path), int(branch), int(clip0), stream())


VLAD_MAX_K, VLAD_MAX_HO, VLAD_MAX_KHO, VLAD_MAX_T = 64, 1024, 16384, 1024       # vl_netvlad_*'s limits (vltf.h)


def _vlad_sizes(who, batch, T, HO, K, **tensors):
    """Every tensor given holds at least what the launch reads or writes of it, where the sizes are ones the launch takes (None and
    sizes outside the limits pass: the C side refuses them by name)."""
    if not (batch > 0 and 2 <= K <= VLAD_MAX_K and 1 <= HO <= VLAD_MAX_HO and K * HO <= VLAD_MAX_KHO and 1 <= T <= VLAD_MAX_T):
        return
    need = dict(s=batch * T * K, a=batch * T * K, ds=batch * T * K, h=batch * T * HO, dh=batch * T * HO, r=batch * K,
                y=batch * K * HO, dy=batch * K * HO, dcp=batch * K * HO, c=K * HO)
    for k, t in tensors.items():
        if t is not None and t.numel() < need[k]:
            raise _ffi.VltfError("%s: %s has %d elements, the launch needs %d" % (who, k, t.numel(), need[k]))


def netvlad_fwd(s, c, h, a, r, y, batch, T, HO, K, seq_len=None):
    """NetVLAD pooling over time (vl_netvlad_fwd): a = softmax_k(s) over the live steps (a may be s), V_k = sum_t a_tk (h_t - c_k),
    y = V_k / max(|V_k|, 1e-6) / sqrt(K), cluster-major.  s, a [batch, T, K]; c [K, HO]; h [batch, T, HO]; r [batch, K];
    y [batch, K HO]; seq_len as temporal_fusion_fwd.  2 <= K <= 64, HO <= 1024, K HO <= 16384, T <= 1024."""
    _f32(s, c, h, a, r, y)
    _dense(s, c, h, a, r, y)
    _vlad_sizes("netvlad_fwd", batch, T, HO, K, s=s, c=c, h=h, a=a, r=r, y=y)
    _ffi.call("vl_netvlad_fwd", _p(s), _p(c), _p(h), None if seq_len is None else _p(_seq_len(seq_len, batch, "netvlad_fwd")),
              _p(a), _p(r), _p(y), batch, T, HO, K, stream())


def netvlad_bwd(dy, h, a, r, y, c, ds, dh, dcp, batch, T, HO, K, seq_len=None):
    """Its backward (vl_netvlad_bwd): ds [batch, T, K], the direct term dh [batch, T, HO] = sum_k a_tk dV_k and the per-clip partials
    dcp [batch, K HO] of c's gradient; dead rows of ds and dh are zeros."""
    _f32(dy, h, a, r, y, c, ds, dh, dcp)
    _dense(dy, h, a, r, y, c, ds, dh, dcp)
    _vlad_sizes("netvlad_bwd", batch, T, HO, K, dy=dy, h=h, a=a, r=r, y=y, c=c, ds=ds, dh=dh, dcp=dcp)
    _ffi.call("vl_netvlad_bwd", _p(dy), _p(h), _p(a), _p(r), _p(y), _p(c),
              None if seq_len is None else _p(_seq_len(seq_len, batch, "netvlad_bwd")), _p(ds), _p(dh), _p(dcp), batch, T, HO, K,
              stream())


def dropout_fwd(x, y, mask, keep, seed):
    _f32(x, y)
    _ffi.call("vl_dropout_fwd", _p(x), _p(y), _p(mask), x.numel(), keep, seed, stream())


def dropout_fwd_st(x, y, mask, keep, state):
    """dropout_fwd with the seed formed on the device from the step state's count (vl_dropout_fwd_st)."""
    _f32(x, y)
    _ffi.call("vl_dropout_fwd_st", _p(x), _p(y), _p(mask), x.numel(), keep, _state(state), stream())


def dropout_bwd(dy, mask, dx, keep):
    _f32(dy, dx)
    _ffi.call("vl_dropout_bwd", _p(dy), _p(mask), _p(dx), dy.numel(), keep, stream())


FC_DROPOUT_GRID_SPAN = 4 * 256 * 4096     # elements one pass of the fc-dropout launches' grid covers (VL_FC_DROPOUT_GRID_CAP)


def fc_dropout_fwd(y, keep, seed, salt):
    """Dropout of a ReLU'd fc output in place, no mask kept (vl_fc_dropout_fwd): element e of y is kept iff the draw of (seed, salt,
    e) falls below keep, and divided by keep."""
    _f32(y); _dense(y)
    _ffi.call("vl_fc_dropout_fwd", _p(y), y.numel(), keep, int(seed), int(salt), stream())


def fc_dropout_fwd_st(y, keep, state, salt):
    """fc_dropout_fwd with the seed formed on the device from the step state's count (vl_fc_dropout_fwd_st)."""
    _f32(y); _dense(y)
    _ffi.call("vl_fc_dropout_fwd_st", _p(y), y.numel(), keep, _state(state), int(salt), stream())


def relu_dropout_grad(d, y, keep, count=None):
    """d = y > 0 ? d / keep : 0 in place: ReluGrad and the dropout gradient of an output fc_dropout_fwd dropped (vl_relu_dropout_grad)."""
    _f32(d, y); _dense(d, y)
    _ffi.call("vl_relu_dropout_grad", _p(d), _p(y), d.numel() if count is None else int(count), keep, stream())


# ---- loss / optimizer ----------------------------------------------------------------------------
def _xent_args(who, cols, logits, labels, dlogits, stats, rows, seq_len=None, T=None, partner=False):
    """The checks the loss wrappers share, for `who` with `cols` columns of stats / rows (partner: the labels are indexed by row, so
    they need the logits' shape) -> (batch, classes, seq_len or None, T or 1)."""
    _f32(logits, dlogits, stats); _dense(logits, labels, dlogits)
    if labels.dtype != torch.int32:
        raise _ffi.VltfError("%s: labels must be int32 one-hot" % who)
    b, c = logits.shape
    if partner and tuple(labels.shape) != (b, c):
        raise _ffi.VltfError("%s: labels must have the logits' shape (the partner's row is found by index)" % who)
    if cols > 2 and stats.numel() < cols:
        raise _ffi.VltfError("%s: stats needs %d floats" % (who, cols))
    if rows is not None:
        _f32(rows)
        if rows.numel() < cols * b:
            raise _ffi.VltfError("%s: rows workspace needs %d*batch floats" % (who, cols))
    if seq_len is None:
        return b, c, None, 1
    if not T or T < 1 or b % int(T):
        raise _ffi.VltfError("%s: seq_len needs T with rows = clips * T (rows %d, T %s)" % (who, b, T))
    return b, c, _seq_len(seq_len, b // int(T), who), int(T)


def softmax_xent(logits, labels, dlogits, stats, grad_scale, rows=None, seq_len=None, T=None):
    """rows: float32 workspace of >= 2*batch elements (per-row losses and hits); without it one workgroup walks the batch.
    seq_len with T: the rows are the steps of batch / T sequences; row b T + t with t >= seq_len[b] is padding -- not read, nothing
    added to `stats`, dlogits 0 (vl_softmax_xent_len; grad_scale is the caller's 1 / live rows)."""
    b, c, sl, t = _xent_args("softmax_xent", 2, logits, labels, dlogits, stats, rows, seq_len, T)
    if sl is not None:
        _ffi.call("vl_softmax_xent_len", _p(logits), _p(labels), _p(dlogits), _p(stats), _p(rows), b, c, grad_scale, _p(sl), t, stream())
        return
    _ffi.call("vl_softmax_xent", _p(logits), _p(labels), _p(dlogits), _p(stats), _p(rows), b, c, grad_scale, stream())


def softmax_xent_ls(logits, labels, dlogits, stats, grad_scale, rows, smoothing, top_k, seq_len=None, T=None):
    """softmax_xent with label smoothing (y' = y (1 - smoothing) + smoothing / classes) and top-k hits in the same launch
    (vl_softmax_xent_ls).  stats: 3 floats (loss sum, top-1 hits, top-k hits; top_k 0 leaves the third alone); rows: None or a float32
    workspace of >= 3*batch elements.  seq_len / T as in softmax_xent."""
    b, c, sl, t = _xent_args("softmax_xent_ls", 3, logits, labels, dlogits, stats, rows, seq_len, T)
    _ffi.call("vl_softmax_xent_ls", _p(logits), _p(labels), _p(dlogits), _p(stats), _p(rows), b, c, grad_scale, _p(sl), t,
              float(smoothing), int(top_k), stream())


def _lam(lam, what):
    """(host lam, device pointer) of a mixup launch: a one-float device tensor is read when the kernel runs, a number is an argument."""
    if torch.is_tensor(lam):
        _f32(lam)
        if lam.numel() != 1:
            raise _ffi.VltfError("%s: a device lam is one float32, got %d elements" % (what, lam.numel()))
        return 0.0, _p(lam)
    return float(lam), None


def mixup_pairs(x, clips, lam):
    """mixup's blend in place (vl_mixup_pairs): x holds `clips` equal clips back to back (any layout inside a clip), float32 or
    bfloat16; clip i and clip clips - 1 - i become lam x_i + (1 - lam) x_p and lam x_p + (1 - lam) x_i.  lam: a number in [0, 1] or
    a one-float device tensor (read when the kernel runs)."""
    if not (torch.is_tensor(x) and x.is_cuda and x.dtype in (F32, torch.bfloat16)):
        raise _ffi.VltfError("mixup_pairs: expected a CUDA/HIP float32 or bfloat16 tensor")
    _dense(x)
    clips = int(clips)
    if clips > 0 and x.numel() % clips:
        raise _ffi.VltfError("mixup_pairs: %d elements are not %d equal clips" % (x.numel(), clips))
    lam_host, lam_dev = _lam(lam, "mixup_pairs")
    _ffi.call("vl_mixup_pairs", _p(x), 0 if x.dtype == F32 else 1, clips, x.numel() // max(clips, 1), lam_host, lam_dev,
              stream())


def _cut_box(box, what):
    """(host pointer, device pointer, keep-alive) of a CutMix launch's box: a six-int32 device tensor is read when the kernel runs,
    a 6-tuple (t0, t1, y0, y1, x0, x1) is six host ints."""
    if torch.is_tensor(box):
        if not (box.is_cuda and box.dtype == torch.int32 and box.numel() == 6 and box.is_contiguous()):
            raise _ffi.VltfError("%s: a device box is six contiguous int32 words (t0, t1, y0, y1, x0, x1)" % what)
        return None, _p(box), None
    try:
        vals = [int(v) for v in box]
        whole = not isinstance(box, (str, bytes)) and all(not isinstance(v, (str, bytes)) and float(v) == int(v) for v in box)
    except (TypeError, ValueError):
        vals, whole = [], False
    if len(vals) != 6 or not whole or any(not -2 ** 31 <= v < 2 ** 31 for v in vals):
        raise _ffi.VltfError("%s: the box is six whole numbers (t0, t1, y0, y1, x0, x1), got %r" % (what, box))
    host = (C.c_int32 * 6)(*vals)
    return C.cast(host, C.c_void_p), None, host


def cutmix_pairs(x0, clips, fpc, out_hw, halo, phase, box):
    """CutMix / VideoMix in place in x0 (vl_cutmix_pairs): x0 is phase_split_shape(clips * fpc, 3, *out_hw, halo, phase), what
    input_prep_u8 writes; the half-open box (t0, t1, y0, y1, x0, x1) of clip i and clip clips - 1 - i is exchanged bit for bit.
    box: a 6-tuple, or a six-int32 device tensor (read when the kernel runs, clamped to the frame)."""
    _f32(x0); _dense(x0)
    clips, fpc = int(clips), int(fpc)
    if clips >= 0 and fpc > 0 and tuple(x0.shape) != phase_split_shape(clips * fpc, 3, out_hw[0], out_hw[1], halo, phase):
        raise _ffi.VltfError("cutmix_pairs: x0 %s is not %d clips of %d frames %s (halo %d, phase %d)"
                             % (tuple(x0.shape), clips, fpc, tuple(out_hw), halo, phase))
    host, dev, keep = _cut_box(box, "cutmix_pairs")
    _ffi.call("vl_cutmix_pairs", _p(x0), clips, fpc, int(out_hw[0]), int(out_hw[1]), int(halo), int(phase), host, dev, stream())
    del keep


ERASE_MODES = ("zero", "clip", "pixel")          # vl_erase_boxes' mode 0, 1, 2
ERASE_SUM_STD = 37837.22723720648                # the standard deviation of the four-field sum: sqrt(4 (65536^2 - 1) / 12)


def erase_scale(std):
    """vl_erase_boxes' scale for a fill of this standard deviation: (float)(std / 37837.22723720648)."""
    return float(np.float32(float(std) / ERASE_SUM_STD))


def _erase_table(table, clips, what):
    if not (torch.is_tensor(table) and table.is_cuda and table.dtype == torch.int32 and table.is_contiguous()
            and (clips < 0 or tuple(table.shape) == (clips, 8))):
        raise _ffi.VltfError("%s: the table is a contiguous device int32 [%d][8] tensor (t0, t1, y0, y1, x0, x1, key_lo, key_hi per clip)"
                             % (what, clips))


def erase_boxes(x0, clips, fpc, out_hw, halo, phase, table, mode, scale):
    """Random erasing in place in x0 (vl_erase_boxes): x0 is phase_split_shape(clips * fpc, 3, *out_hw, halo, phase), what
    input_prep_u8 writes; clip i's half-open box (row i of table, read when the kernel runs and clamped to the frame) is overwritten
    in all channels.  table: device int32 [clips][8] = (t0, t1, y0, y1, x0, x1, key_lo, key_hi).  mode: 0 zero, 1 one value per
    (clip, channel), 2 one per element (ERASE_MODES).  scale: erase_scale(std)."""
    _f32(x0); _dense(x0)
    clips, fpc = int(clips), int(fpc)
    if clips >= 0 and fpc > 0 and tuple(x0.shape) != phase_split_shape(clips * fpc, 3, out_hw[0], out_hw[1], halo, phase):
        raise _ffi.VltfError("erase_boxes: x0 %s is not %d clips of %d frames %s (halo %d, phase %d)"
                             % (tuple(x0.shape), clips, fpc, tuple(out_hw), halo, phase))
    _erase_table(table, clips, "erase_boxes")
    _ffi.call("vl_erase_boxes", _p(x0), clips, fpc, int(out_hw[0]), int(out_hw[1]), int(halo), int(phase), _p(table), int(mode), float(scale),
              stream())


def softmax_xent_mix(logits, labels, dlogits, stats, grad_scale, rows, rows_per_clip, smoothing, top_k, lam):
    """softmax_xent_ls on the labels of clips blended by mixup_pairs (vl_softmax_xent_mix): y' = lam y + (1 - lam) y_partner ahead of
    the smoothing, the partner being the same row of the clip mirrored in the batch; hits against the row's own label.  logits are
    clips of rows_per_clip rows.  stats: 3 floats; rows: None or >= 3*batch floats; lam as in mixup_pairs."""
    b, c, _, _ = _xent_args("softmax_xent_mix", 3, logits, labels, dlogits, stats, rows, partner=True)
    lam_host, lam_dev = _lam(lam, "softmax_xent_mix")
    _ffi.call("vl_softmax_xent_mix", _p(logits), _p(labels), _p(dlogits), _p(stats), _p(rows), b, c, grad_scale, int(rows_per_clip),
              float(smoothing), int(top_k), lam_host, lam_dev, stream())


def softmax_xent_wf(logits, labels, dlogits, stats, grad_scale, rows, smoothing, top_k, class_weights=None, gamma=0.0, seq_len=None,
                    T=None, rows_per_clip=1, lam=1.0):
    """softmax_xent_ls / softmax_xent_mix with class weights and the focal loss in the same launch (vl_softmax_xent_wf):
    loss = sum_c w_c y'_c (1 - p_c)^gamma (-log p_c), normalised by the caller's row count (grad_scale).  class_weights: None (ones) or
    a float32 device tensor of `classes` elements, read when the kernel runs; gamma >= 0.  seq_len / T as in softmax_xent_ls;
    rows_per_clip / lam as in softmax_xent_mix (1 and 1.0: no partner row); the two do not combine.  stats: 3 floats; rows: None or
    >= 3*batch floats."""
    mixed = int(rows_per_clip) != 1 or torch.is_tensor(lam) or float(lam) != 1.0
    b, c, sl, t = _xent_args("softmax_xent_wf", 3, logits, labels, dlogits, stats, rows, seq_len, T, partner=mixed)
    if class_weights is not None:
        _f32(class_weights); _dense(class_weights)
        if class_weights.numel() != c:
            raise _ffi.VltfError("softmax_xent_wf: class_weights holds %d floats for %d classes" % (class_weights.numel(), c))
    lam_host, lam_dev = _lam(lam, "softmax_xent_wf")
    _ffi.call("vl_softmax_xent_wf", _p(logits), _p(labels), _p(dlogits), _p(stats), _p(rows), b, c, grad_scale, _p(sl), t,
              int(rows_per_clip), float(smoothing), int(top_k), lam_host, lam_dev, _p(class_weights), float(gamma), stream())


def sigmoid_xent(logits, labels, dlogits, stats, grad_scale, rows, smoothing=0.0, pos_weights=None, gamma=0.0, seq_len=None, T=None,
                 rows_per_clip=1, lam=1.0):
    """The multi-label loss launch (vl_sigmoid_xent): independent sigmoids per class on multi-hot int32 labels, the row loss the MEAN
    over the classes, dlogits = dl/dz * grad_scale / classes.  smoothing: t' = t (1 - smoothing) + smoothing / 2, after the mixup
    blend.  pos_weights: None (ones) or a float32 device tensor of `classes` elements, the weight of each class's positive term, read
    when the kernel runs; gamma >= 0: the sigmoid focal loss.  seq_len / T as in softmax_xent_ls; rows_per_clip / lam as in
    softmax_xent_mix (1 and 1.0: no partner row); the two do not combine.  stats: 3 floats (loss sum, hit@1 rows, exact-match rows);
    rows: None or >= 3*batch floats."""
    mixed = int(rows_per_clip) != 1 or torch.is_tensor(lam) or float(lam) != 1.0
    b, c, sl, t = _xent_args("sigmoid_xent", 3, logits, labels, dlogits, stats, rows, seq_len, T, partner=mixed)
    if pos_weights is not None:
        _f32(pos_weights); _dense(pos_weights)
        if pos_weights.numel() != c:
            raise _ffi.VltfError("sigmoid_xent: pos_weights holds %d floats for %d classes" % (pos_weights.numel(), c))
    lam_host, lam_dev = _lam(lam, "sigmoid_xent")
    _ffi.call("vl_sigmoid_xent", _p(logits), _p(labels), _p(dlogits), _p(stats), _p(rows), b, c, grad_scale, _p(sl), t,
              int(rows_per_clip), float(smoothing), lam_host, lam_dev, _p(pos_weights), float(gamma), stream())


def sumsq(g, out, ws, accumulate=False):
    _f32(g, out, ws)
    if ws.numel() < 1024:
        raise _ffi.VltfError("sumsq: workspace needs 1024 floats")
    _ffi.call("vl_sumsq", _p(g), g.numel(), _p(out), _p(ws), int(accumulate), stream())


def _skip_word(skip):
    if skip is not None and not (skip.is_cuda and skip.dtype == torch.int32 and skip.numel() >= 1):
        raise _ffi.VltfError("skip must be a CUDA/HIP int32 tensor (one word)")
    return _p(skip)


def sgd_apply(w, g, lr, clip_norm=0.0, sumsq_t=None, gscale=1.0, skip=None):
    """skip: optional device word (int32); non-zero at execution time = the update is dropped (step_guard)."""
    _f32(w, g, sumsq_t)
    _ffi.call("vl_sgd_apply", _p(w), _p(g), w.numel(), lr, clip_norm, _p(sumsq_t), gscale, _skip_word(skip), stream())


def adam_apply(w, g, m, v, lr, step, clip_norm=0.0, sumsq_t=None, gscale=1.0, skip=None):
    _f32(w, g, m, v, sumsq_t)
    _ffi.call("vl_adam_apply", _p(w), _p(g), _p(m), _p(v), w.numel(), lr, clip_norm, _p(sumsq_t), gscale, step, _skip_word(skip), stream())


# ---- step state (vltf.h: vl_step_state): the scalars a replayed step reads from device memory ----------------------------------
def step_state(device):
    """A zeroed device block for vl_step_state (int32 words)."""
    n = int(_ffi.lib().vl_step_state_bytes())
    return torch.zeros((n + 3) // 4, dtype=torch.int32, device=device)


def _state(state):
    if state is None or not (state.is_cuda and state.dtype == torch.int32 and state.numel() * 4 >= int(_ffi.lib().vl_step_state_bytes())):
        raise _ffi.VltfError("expected a step state from step_state()")
    return _p(state)


def step_state_set(state, step, lr, tag_origin):
    """state = (step, lr, tag_origin, Adam's step size for count step + 1), written on the stream (vl_step_state_set)."""
    _ffi.call("vl_step_state_set", _state(state), int(step), lr, int(tag_origin), stream())


def step_state_set_micro(state, update_step, draw_step, lr, tag_origin):
    """step_state_set for a micro-step of an accumulated update: the state's count (the dropout seed's input) = draw_step, Adam's step
    size that of count update_step + 1 (vl_step_state_set_micro)."""
    _ffi.call("vl_step_state_set_micro", _state(state), int(update_step), int(draw_step), lr, int(tag_origin), stream())


def step_state_set_ema(state, rate):
    """state.ema_rate = rate, and nothing else of the block, written on the stream (vl_step_state_set_ema)."""
    _ffi.call("vl_step_state_set_ema", _state(state), rate, stream())


def sgd_apply_st(w, g, state, clip_norm=0.0, sumsq_t=None, gscale=1.0, skip=None):
    """sgd_apply with lr read from the step state."""
    _f32(w, g, sumsq_t)
    _ffi.call("vl_sgd_apply_st", _p(w), _p(g), w.numel(), _state(state), clip_norm, _p(sumsq_t), gscale, _skip_word(skip), stream())


def adam_apply_st(w, g, m, v, state, clip_norm=0.0, sumsq_t=None, gscale=1.0, skip=None):
    """adam_apply with the step size for the state's count + 1 read from the step state."""
    _f32(w, g, m, v, sumsq_t)
    _ffi.call("vl_adam_apply_st", _p(w), _p(g), _p(m), _p(v), w.numel(), _state(state), clip_norm, _p(sumsq_t), gscale, _skip_word(skip),
              stream())


# ---- tiered update (vltf.h: vl_lr_tier): per-range learning-rate multipliers, gaps untouched --------------------------------------
def _tiers(tiers):
    """[(begin, end, lr_mult)] -> (vl_lr_tier array, count); the library validates the table."""
    tiers = list(tiers)
    arr = (_ffi.LrTier * max(len(tiers), 1))()
    for k, (lo, hi, mult) in enumerate(tiers):
        arr[k].begin, arr[k].end, arr[k].lr_mult = int(lo), int(hi), float(mult)
    return arr, len(tiers)


def sumsq_tiers(g, tiers, out, ws):
    """out[0] = sum g^2 over the elements inside the tiers; elements outside are not read."""
    _f32(g, out, ws)
    if ws.numel() < 1024:
        raise _ffi.VltfError("sumsq_tiers: workspace needs 1024 floats")
    arr, n = _tiers(tiers)
    _ffi.call("vl_sumsq_tiers", _p(g), g.numel(), arr, n, _p(out), _p(ws), stream())


def l2_regularize(w, g, ranges, out, ws):
    """L2 weight decay in the norm's launch (vltf.h: vl_l2_regularize).  ranges = [(begin, end, decay)]: inside a range with decay > 0
    g becomes g + decay * w IN PLACE; out[0] = sum of the regularised g^2 over every range, out[1] = sum (decay / 2) w^2.  A range with
    decay 0 is only summed (w not read, g not written); elements outside every range are not touched."""
    _f32(w, g, out, ws)
    if g.numel() != w.numel():
        raise _ffi.VltfError("l2_regularize: w and g must have one element count")
    if out.numel() < 2:
        raise _ffi.VltfError("l2_regularize: out needs 2 floats")
    if ws.numel() < 2048:
        raise _ffi.VltfError("l2_regularize: workspace needs 2048 floats")
    ranges = list(ranges)
    arr = (_ffi.DecayRange * max(len(ranges), 1))()
    for k, (lo, hi, decay) in enumerate(ranges):
        arr[k].begin, arr[k].end, arr[k].decay = int(lo), int(hi), float(decay)
    _ffi.call("vl_l2_regularize", _p(w), _p(g), w.numel(), arr, len(ranges), _p(out), _p(ws), stream())


# ---- per-variable statistics (vltf.h: vl_tensor_stats) ------------------------------------------------------------------------------
STAT_CHUNK, MAX_STAT_SEGMENTS = _ffi.STAT_CHUNK, _ffi.MAX_STAT_SEGMENTS
STAT_ROW_BYTES = 64
# a vl_tensor_stat row as numpy reads it from the bytes of `out`
STAT_DTYPE = np.dtype([("g_sum", "<f8"), ("g_sumsq", "<f8"), ("w_sum", "<f8"), ("w_sumsq", "<f8"),
                       ("g_min", "<f4"), ("g_max", "<f4"), ("w_min", "<f4"), ("w_max", "<f4"),
                       ("g_nonfinite", "<u4"), ("w_nonfinite", "<u4"), ("g_zero", "<u4"), ("reserved", "<u4")])


def _stat_segments(segments):
    """[(begin, end)] or [(name, begin, end)] -> [(begin, end)]."""
    return [(int(s[-2]), int(s[-1])) for s in segments]


def stat_chunk_plan(segments):
    """(first chunk index of every segment, chunks of the table): a segment is cut into chunks of STAT_CHUNK elements, the last one
    short, and chunks never span segments.  Host only; the library derives the same plan from the table it is handed."""
    first, chunks = [], 0
    for lo, hi in _stat_segments(segments):
        first.append(chunks)
        chunks += -(-(hi - lo) // STAT_CHUNK)
    return first, chunks


def _stat_slices(segments):
    segs = _stat_segments(segments)
    if not segs:
        raise _ffi.VltfError("tensor_stats: the segment table is empty")
    return [segs[i:i + MAX_STAT_SEGMENTS] for i in range(0, len(segs), MAX_STAT_SEGMENTS)]


def _stat_array(segs):
    arr = (_ffi.StatSegment * len(segs))()
    for k, (lo, hi) in enumerate(segs):
        arr[k].begin, arr[k].end = lo, hi
    return arr


def tensor_stats_ws_bytes(segments):
    """Bytes of workspace tensor_stats needs for this table: the largest requirement over its slices of MAX_STAT_SEGMENTS entries.
    Host only.  A table the library refuses raises."""
    need = 0
    for segs in _stat_slices(segments):
        n = int(_ffi.lib().vl_tensor_stats_ws_bytes(_stat_array(segs), len(segs)))
        if n == 0:
            raise _ffi.VltfError("tensor_stats_ws_bytes: %s" % (_ffi.lib().vl_last_error() or b"bad segment table").decode())
        need = max(need, n)
    return need


def tensor_stats(w, g, segments, out, ws):
    """One row of statistics per segment of the flat buffers w and g (vltf.h: vl_tensor_stats); read-only on both.  segments =
    [(begin, end)] or [(name, begin, end)], any number: ceil(n / MAX_STAT_SEGMENTS) launches over consecutive slices of the table and
    of out.  out: uint8 device tensor of STAT_ROW_BYTES per segment (stat_rows reads it), ws: uint8 device tensor of
    tensor_stats_ws_bytes(segments); both are overwritten, neither needs zeroing."""
    _f32(w, g)
    if g.numel() != w.numel():
        raise _ffi.VltfError("tensor_stats: w and g must have one element count")
    slices = _stat_slices(segments)
    total = sum(len(s) for s in slices)
    for t, what in ((out, "out"), (ws, "ws")):
        if t is None or not (t.is_cuda and t.dtype == torch.uint8 and t.is_contiguous()):
            raise _ffi.VltfError("tensor_stats: %s must be a contiguous CUDA/HIP uint8 tensor" % what)
    if out.numel() < total * STAT_ROW_BYTES:
        raise _ffi.VltfError("tensor_stats: out needs %d bytes (%d per segment), has %d" % (total * STAT_ROW_BYTES, STAT_ROW_BYTES, out.numel()))
    done = 0
    for segs in slices:
        _ffi.call("vl_tensor_stats", _p(w), _p(g), w.numel(), _stat_array(segs), len(segs), out.data_ptr() + done * STAT_ROW_BYTES, _p(ws),
                  ws.numel(), stream())
        done += len(segs)


def stat_rows(out, n):
    """The first n rows of a tensor_stats `out` on the host, as a numpy array of STAT_DTYPE (synchronises through the copy)."""
    return out[:n * STAT_ROW_BYTES].cpu().numpy().view(STAT_DTYPE).copy()


ACC_STORE, ACC_ADD, ACC_FINAL = 0, 1, 2


def grad_accumulate(acc, g, mode, ranges=None):
    """Gradient accumulation (vltf.h: vl_grad_accumulate).  mode ACC_STORE: acc = g; ACC_ADD: acc = acc + g; ACC_FINAL: g = acc + g.
    ranges = [(begin, end, lr_mult)] (plan.tiers; the factor is ignored) or None for everything; elements outside every range are
    not touched in either buffer.  One launch."""
    _f32(acc, g)
    if acc.numel() != g.numel():
        raise _ffi.VltfError("grad_accumulate: acc and g must have one element count")
    if ranges is None:
        arr, n = None, 0
    else:
        arr, n = _tiers(ranges)
    _ffi.call("vl_grad_accumulate", _p(acc), _p(g), g.numel(), int(mode), arr, n, stream())


def sgd_apply_tiers(w, g, tiers, lr, clip_norm=0.0, sumsq_t=None, gscale=1.0, skip=None):
    """sgd_apply over the tiers [(begin, end, lr_mult)] only, each with lr * lr_mult: one launch."""
    _f32(w, g, sumsq_t)
    arr, n = _tiers(tiers)
    _ffi.call("vl_sgd_apply_tiers", _p(w), _p(g), w.numel(), lr, clip_norm, _p(sumsq_t), gscale, _skip_word(skip), arr, n, stream())


def adam_apply_tiers(w, g, m, v, tiers, lr, step, clip_norm=0.0, sumsq_t=None, gscale=1.0, skip=None):
    _f32(w, g, m, v, sumsq_t)
    arr, n = _tiers(tiers)
    _ffi.call("vl_adam_apply_tiers", _p(w), _p(g), _p(m), _p(v), w.numel(), lr, clip_norm, _p(sumsq_t), gscale, step, _skip_word(skip),
              arr, n, stream())


def sgd_apply_tiers_st(w, g, tiers, state, clip_norm=0.0, sumsq_t=None, gscale=1.0, skip=None):
    _f32(w, g, sumsq_t)
    arr, n = _tiers(tiers)
    _ffi.call("vl_sgd_apply_tiers_st", _p(w), _p(g), w.numel(), _state(state), clip_norm, _p(sumsq_t), gscale, _skip_word(skip), arr, n,
              stream())


def adam_apply_tiers_st(w, g, m, v, tiers, state, clip_norm=0.0, sumsq_t=None, gscale=1.0, skip=None):
    _f32(w, g, m, v, sumsq_t)
    arr, n = _tiers(tiers)
    _ffi.call("vl_adam_apply_tiers_st", _p(w), _p(g), _p(m), _p(v), w.numel(), _state(state), clip_norm, _p(sumsq_t), gscale,
              _skip_word(skip), arr, n, stream())


def _momentum_sizes(w, g, accum):
    if g.numel() != w.numel() or (accum is not None and accum.numel() != w.numel()):
        raise _ffi.VltfError("momentum_apply: w, g and accum must have one element count")


def momentum_apply(w, g, accum, lr, momentum, nesterov=False, clip_norm=0.0, sumsq_t=None, gscale=1.0, skip=None, tiers=None):
    """SGD with momentum (tf.train.MomentumOptimizer; vltf.h: vl_momentum_apply): accum = momentum * accum + clipped g, then
    w -= lr * accum (nesterov: lr * (clipped g + momentum * accum)).  tiers None: the whole buffer; else as sgd_apply_tiers."""
    _f32(w, g, accum, sumsq_t)
    _momentum_sizes(w, g, accum)
    arr, n = (None, 0) if tiers is None else _tiers(tiers)
    _ffi.call("vl_momentum_apply", _p(w), _p(g), _p(accum), w.numel(), lr, momentum, int(bool(nesterov)), clip_norm, _p(sumsq_t), gscale,
              _skip_word(skip), arr, n, stream())


def momentum_apply_st(w, g, accum, state, momentum, nesterov=False, clip_norm=0.0, sumsq_t=None, gscale=1.0, skip=None, tiers=None):
    """momentum_apply with lr read from the step state."""
    _f32(w, g, accum, sumsq_t)
    _momentum_sizes(w, g, accum)
    arr, n = (None, 0) if tiers is None else _tiers(tiers)
    _ffi.call("vl_momentum_apply_st", _p(w), _p(g), _p(accum), w.numel(), _state(state), momentum, int(bool(nesterov)), clip_norm,
              _p(sumsq_t), gscale, _skip_word(skip), arr, n, stream())


# ---- LARS (vltf.h: vl_lars_trust, vl_lars_apply): per-variable trust ratios on the device, the momentum update through them ---------------
def lars_trust(rows, decay, trust, eeta, eps=0.0, clip_norm=0.0, sumsq_t=None, gscale=1.0):
    """trust[k] = eeta * |w_k| / (sc * |g_k| + decay[k] * |w_k| + eps) from row k of a tensor_stats `out` (rows: its uint8 tensor), or 1
    where a norm is 0 or the row counts a non-finite element; sc is the clip scale the update forms from clip_norm, sumsq_t and gscale.
    decay: one coefficient per row, on the host, any number of rows: ceil(n / MAX_STAT_SEGMENTS) launches over consecutive slices, as
    tensor_stats.  trust: float32 device tensor of at least len(decay) entries, overwritten."""
    _f32(trust, sumsq_t)
    decay = [float(d) for d in decay]
    n = len(decay)
    if n == 0:
        raise _ffi.VltfError("lars_trust: no segments")
    if rows is None or not (rows.is_cuda and rows.dtype == torch.uint8 and rows.is_contiguous()) or rows.numel() < n * STAT_ROW_BYTES:
        raise _ffi.VltfError("lars_trust: rows must be a contiguous CUDA/HIP uint8 tensor of %d bytes per segment" % STAT_ROW_BYTES)
    if trust.numel() < n:
        raise _ffi.VltfError("lars_trust: trust needs %d floats, has %d" % (n, trust.numel()))
    for lo in range(0, n, MAX_STAT_SEGMENTS):
        part = decay[lo:lo + MAX_STAT_SEGMENTS]
        arr = (_ffi.f32 * len(part))(*part)
        _ffi.call("vl_lars_trust", rows.data_ptr() + lo * STAT_ROW_BYTES, len(part), float(eeta), float(eps), arr, clip_norm, _p(sumsq_t),
                  gscale, trust.data_ptr() + 4 * lo, stream())


def _lars_slices(ranges):
    """[(begin, end, lr_mult, trust_index)] -> [(vl_lars_range array, count)] over consecutive slices of MAX_STAT_SEGMENTS entries; the
    library validates each."""
    ranges = list(ranges)
    out = []
    for lo in range(0, max(len(ranges), 1), MAX_STAT_SEGMENTS):
        part = ranges[lo:lo + MAX_STAT_SEGMENTS]
        arr = (_ffi.LarsRange * max(len(part), 1))()
        for k, (a, b, mult, ti) in enumerate(part):
            arr[k].begin, arr[k].end, arr[k].lr_mult, arr[k].trust_index = int(a), int(b), float(mult), int(ti)
        out.append((arr, len(part)))
    return out


def _lars_trust_arg(trust):
    if trust is None:
        return None, 0
    _f32(trust)
    return _p(trust), trust.numel()


def lars_apply(w, g, accum, ranges, trust, lr, momentum, nesterov=False, clip_norm=0.0, sumsq_t=None, gscale=1.0, skip=None):
    """momentum_apply over ranges = [(begin, end, lr_mult, trust_index)], each with lr * lr_mult * trust[trust_index] (index -1: trust 1,
    nothing read); trust is read on the device when the launch runs (lars_trust).  One launch per MAX_STAT_SEGMENTS ranges."""
    _f32(w, g, accum, sumsq_t)
    _momentum_sizes(w, g, accum)
    tp, nt = _lars_trust_arg(trust)
    for arr, n in _lars_slices(ranges):
        _ffi.call("vl_lars_apply", _p(w), _p(g), _p(accum), w.numel(), lr, momentum, int(bool(nesterov)), clip_norm, _p(sumsq_t), gscale,
                  _skip_word(skip), arr, n, tp, nt, stream())


def lars_apply_st(w, g, accum, ranges, trust, state, momentum, nesterov=False, clip_norm=0.0, sumsq_t=None, gscale=1.0, skip=None):
    """lars_apply with lr read from the step state."""
    _f32(w, g, accum, sumsq_t)
    _momentum_sizes(w, g, accum)
    tp, nt = _lars_trust_arg(trust)
    for arr, n in _lars_slices(ranges):
        _ffi.call("vl_lars_apply_st", _p(w), _p(g), _p(accum), w.numel(), _state(state), momentum, int(bool(nesterov)), clip_norm,
                  _p(sumsq_t), gscale, _skip_word(skip), arr, n, tp, nt, stream())


# ---- LAMB (vltf.h: vl_lamb_moments, vl_lamb_apply): Adam's moments, per-tensor trust ratios on the device, decoupled decay ---------------
LAMB_ROW_BYTES = 24
# a vl_lamb_row as numpy reads it from the bytes of `rows`
LAMB_ROW_DTYPE = np.dtype([("w_sumsq", "<f8"), ("u_sumsq", "<f8"), ("nonfinite", "<u4"), ("reserved", "<u4")])


def _lamb_slices(ranges, who):
    """[(begin, end, lr_mult, decay, trust_index)] -> [(vl_lamb_range array, count)] over consecutive slices of MAX_STAT_SEGMENTS entries;
    the library validates each."""
    ranges = list(ranges)
    if not ranges:
        raise _ffi.VltfError("%s: the range table is empty" % who)
    out = []
    for lo in range(0, len(ranges), MAX_STAT_SEGMENTS):
        part = ranges[lo:lo + MAX_STAT_SEGMENTS]
        arr = (_ffi.LambRange * len(part))()
        for k, (a, b, mult, decay, ti) in enumerate(part):
            arr[k].begin, arr[k].end, arr[k].lr_mult, arr[k].decay, arr[k].trust_index = int(a), int(b), float(mult), float(decay), int(ti)
        out.append((arr, len(part)))
    return out


def lamb_moments_ws_bytes(ranges):
    """Bytes of workspace lamb_moments needs for this table: the largest requirement over its slices.  Host only.  A table the library
    refuses raises."""
    need = 0
    for arr, n in _lamb_slices(ranges, "lamb_moments_ws_bytes"):
        b = int(_ffi.lib().vl_lamb_moments_ws_bytes(arr, n))
        if b == 0:
            raise _ffi.VltfError("lamb_moments_ws_bytes: %s" % (_ffi.lib().vl_last_error() or b"bad range table").decode())
        need = max(need, b)
    return need


def _lamb_moments_args(w, g, m, v, rows, trust, ws, sumsq_t, who):
    if any(t is None for t in (w, g, m, v)):
        raise _ffi.VltfError("%s: w, g, m and v must be tensors" % who)
    _f32(w, g, m, v, sumsq_t)
    if not (g.numel() == w.numel() == m.numel() == v.numel()):
        raise _ffi.VltfError("%s: w, g, m and v must have one element count" % who)
    if ws is None or not (ws.is_cuda and ws.dtype == torch.uint8 and ws.is_contiguous()):
        raise _ffi.VltfError("%s: ws must be a contiguous CUDA/HIP uint8 tensor" % who)
    if trust is None:
        return None, None, 0
    _f32(trust)
    nt = trust.numel()
    if rows is None or not (rows.is_cuda and rows.dtype == torch.uint8 and rows.is_contiguous()) or rows.numel() < nt * LAMB_ROW_BYTES:
        raise _ffi.VltfError("%s: rows must be a contiguous CUDA/HIP uint8 tensor of %d bytes per entry of trust" % (who, LAMB_ROW_BYTES))
    return _p(rows), _p(trust), nt


def lamb_moments(w, g, m, v, ranges, rows, trust, ws, c1, c2, eps, clip_norm=0.0, sumsq_t=None, gscale=1.0, skip=None):
    """The first launch of a LAMB update (vltf.h: vl_lamb_moments).  ranges = [(begin, end, lr_mult, decay, trust_index)], any number: one
    launch per MAX_STAT_SEGMENTS entries, all indexing the one rows / trust pair.  Inside every range m and v become this update's
    moments (adam_apply's bits); for each range with an index, rows[index] = (sum w^2, sum u^2, non-finite count) in fp64 and
    trust[index] = |w| / |u| (1 where a norm is 0 or an element is not finite).  w and g are read only.  rows: uint8 device tensor of
    LAMB_ROW_BYTES per entry of trust (lamb_rows reads it), trust: float32, ws: uint8 of lamb_moments_ws_bytes(ranges); rows and trust
    may be None for a table without an index.  c1, c2: engine.lamb_corrections."""
    rp, tp, nt = _lamb_moments_args(w, g, m, v, rows, trust, ws, sumsq_t, "lamb_moments")
    for arr, n in _lamb_slices(ranges, "lamb_moments"):
        _ffi.call("vl_lamb_moments", _p(w), _p(g), _p(m), _p(v), w.numel(), c1, c2, eps, clip_norm, _p(sumsq_t), gscale, _skip_word(skip),
                  arr, n, rp, tp, nt, _p(ws), ws.numel(), stream())


def lamb_moments_st(w, g, m, v, ranges, rows, trust, ws, state, eps, clip_norm=0.0, sumsq_t=None, gscale=1.0, skip=None):
    """lamb_moments with c1 and c2 read from the step state (step_state_set_lamb)."""
    rp, tp, nt = _lamb_moments_args(w, g, m, v, rows, trust, ws, sumsq_t, "lamb_moments_st")
    for arr, n in _lamb_slices(ranges, "lamb_moments_st"):
        _ffi.call("vl_lamb_moments_st", _p(w), _p(g), _p(m), _p(v), w.numel(), _state(state), eps, clip_norm, _p(sumsq_t), gscale,
                  _skip_word(skip), arr, n, rp, tp, nt, _p(ws), ws.numel(), stream())


def lamb_rows(rows, n):
    """The first n rows of a lamb_moments `rows` on the host, as a numpy array of LAMB_ROW_DTYPE (synchronises through the copy)."""
    return rows[:n * LAMB_ROW_BYTES].cpu().numpy().view(LAMB_ROW_DTYPE).copy()


def _lamb_apply_args(w, m, v, trust, who):
    if any(t is None for t in (w, m, v)):
        raise _ffi.VltfError("%s: w, m and v must be tensors" % who)
    _f32(w, m, v)
    if not (w.numel() == m.numel() == v.numel()):
        raise _ffi.VltfError("%s: w, m and v must have one element count" % who)
    return _lars_trust_arg(trust)


def lamb_apply(w, m, v, ranges, trust, lr, c1, c2, eps, skip=None):
    """The second launch of a LAMB update (vltf.h: vl_lamb_apply): w <- w - (lr * lr_mult * trust[trust_index]) * u over the ranges of
    lamb_moments, u recomputed from the stored moments and the unchanged w; index -1: trust 1, nothing read.  trust is read on the device
    when the launch runs.  One launch per MAX_STAT_SEGMENTS ranges."""
    tp, nt = _lamb_apply_args(w, m, v, trust, "lamb_apply")
    for arr, n in _lamb_slices(ranges, "lamb_apply"):
        _ffi.call("vl_lamb_apply", _p(w), _p(m), _p(v), w.numel(), lr, c1, c2, eps, _skip_word(skip), arr, n, tp, nt, stream())


def lamb_apply_st(w, m, v, ranges, trust, state, eps, skip=None):
    """lamb_apply with lr, c1 and c2 read from the step state."""
    tp, nt = _lamb_apply_args(w, m, v, trust, "lamb_apply_st")
    for arr, n in _lamb_slices(ranges, "lamb_apply_st"):
        _ffi.call("vl_lamb_apply_st", _p(w), _p(m), _p(v), w.numel(), _state(state), eps, _skip_word(skip), arr, n, tp, nt, stream())


def step_state_set_lamb(state, c1, c2):
    """The state's two LAMB words = (c1, c2), and nothing else of the block, written on the stream (vl_step_state_set_lamb)."""
    _ffi.call("vl_step_state_set_lamb", _state(state), c1, c2, stream())


def _ema_sizes(shadow, w):
    if shadow.numel() != w.numel():
        raise _ffi.VltfError("ema_update: shadow and w must have one element count")


def ema_update(shadow, w, rate, skip=None, ranges=None):
    """Exponential moving average of the weights (tf.train.ExponentialMovingAverage; vltf.h: vl_ema_update): shadow += rate * (w - shadow)
    with rate = 1 - decay.  ranges = [(begin, end, lr_mult)] (plan.tiers; the factor is ignored) or None for everything; elements outside
    every range are not touched in either buffer.  skip: as sgd_apply.  One launch."""
    _f32(shadow, w)
    _ema_sizes(shadow, w)
    arr, n = (None, 0) if ranges is None else _tiers(ranges)
    _ffi.call("vl_ema_update", _p(shadow), _p(w), w.numel(), rate, _skip_word(skip), arr, n, stream())


def ema_update_st(shadow, w, state, skip=None, ranges=None):
    """ema_update with the rate read from the step state (step_state_set_ema)."""
    _f32(shadow, w)
    _ema_sizes(shadow, w)
    arr, n = (None, 0) if ranges is None else _tiers(ranges)
    _ffi.call("vl_ema_update_st", _p(shadow), _p(w), w.numel(), _state(state), _skip_word(skip), arr, n, stream())


def step_guard(skip, *lstm_workspaces):
    """skip[0] = 1 if a cluster-form LSTM launch on any of the workspaces has timed out since its status was last read (the word is
    sticky, lstm_seq_check reads and resets it), else 0 -- on the stream, no host round trip.  Hand `skip` to sgd_apply / adam_apply:
    a step whose recurrence gave up (its results are invalid by the kernel's own contract) must not reach the weights."""
    _skip_word(skip)
    first = True                                  # no workspace: the word keeps the 0 it was created with (nothing ever sets it)
    for ws in lstm_workspaces:
        if ws is not None:
            _ffi.call("vl_status_or", _p(skip), _p(ws), int(first), stream())
            first = False
    return skip


def fill(t, value):
    _f32(t)
    _ffi.call("vl_fill", _p(t), t.numel(), value, stream())


CONV_MATH = {"f32": 0, "bf16": 1, "bf16x3": 3, "bf16x6": 6}


def set_conv_math(name):
    """Arithmetic of the conv contractions (vl_set_conv_math): "f32" (default), "bf16x3" (split bf16 products) or "bf16" (plain
    bf16 products: reduced precision), both opt-in."""
    if name not in CONV_MATH:
        raise _ffi.VltfError("conv math must be one of %s, not %r" % (sorted(CONV_MATH), name))
    _ffi.call("vl_set_conv_math", CONV_MATH[name])


def conv_math():
    return {v: k for k, v in CONV_MATH.items()}[int(_ffi.lib().vl_conv_math())]


def conv_set_row_classes(on=True):
    """Test hook: off runs the many-frames fp32 conv forward / dgrad launches in the flat pixel order (every tap of every tile, the
    padding taps included) instead of the row-class order; results are bitwise the same."""
    _ffi.call("vl_conv_set_row_classes", int(bool(on)))


def conv_set_stage_depth(rows=0):
    """Test hook: 16 or 32 forces the reduction-stage depth of the 16x16-MFMA LDS-DMA conv kernel (three or two workgroups per CU),
    0 returns the choice to the dispatcher; results are bitwise the same."""
    _ffi.call("vl_conv_set_stage_depth", int(rows))


def conv_last_launch():
    """Kernel form of the latest fp32 conv forward / dgrad call: tile height * 100 + stage depth for an LDS-DMA launch (4816, 4832,
    9616, 9632, 12832), 0 for any other kernel."""
    return int(_ffi.lib().vl_conv_last_launch())


def relu_grad(d, y, count=None):
    """d = y > 0 ? d : 0 in place over the first `count` elements."""
    _f32(d, y); _dense(d, y)
    _ffi.call("vl_relu_grad", _p(d), _p(y), d.numel() if count is None else int(count), stream())


# ---- tensor-list plumbing (tf_util.py:99-192) ----------------------------------------------------------------------------------
def copy2d(src, dst, rows, cols, src_ld=None, dst_ld=None):
    """dst[r, :cols] = src[r, :cols]; src / dst may be views (data_ptr + row strides are used); src_ld = 0 repeats one row."""
    _f32(src, dst)
    _ffi.call("vl_copy2d", _p(src), cols if src_ld is None else int(src_ld), _p(dst), cols if dst_ld is None else int(dst_ld),
              int(rows), int(cols), stream())


ELTWISE_OP = {"add": 0, "avg": 1, "maximum": 2}


def eltwise2(a, b, out, op, count=None):
    _f32(a, b, out)
    _ffi.call("vl_eltwise2", _p(a), _p(b), _p(out), a.numel() if count is None else int(count), ELTWISE_OP[op], stream())


def max2_grad(a, b, d, da, db, count=None):
    _f32(a, b, d, da, db)
    _ffi.call("vl_max2_grad", _p(a), _p(b), _p(d), _p(da), _p(db), a.numel() if count is None else int(count), stream())


FUSE_OP = {"avg": 0, "maximum": 1}


def _ptr_list(ts):
    arr = (C.c_void_p * len(ts))()
    for i, t in enumerate(ts):
        arr[i] = None if t is None else t.data_ptr()
    return arr


def fuse_n(ins, out, method, count=None):
    """out = mean | maximum over the list `ins` of equally shaped tensors (apply_tensor_list_fusion avg | maximum, tf_util.py:142-145)."""
    _f32(out, *ins)
    if not 1 <= len(ins) <= 8:
        raise _ffi.VltfError("fuse_n: 1..8 inputs, got %d" % len(ins))
    _ffi.call("vl_fuse_n", _ptr_list(ins), len(ins), _p(out), ins[0].numel() if count is None else int(count), FUSE_OP[method], stream())


def fuse_n_grad(ins, d, dins, method, count=None):
    """dins[i] (None = not wanted) = gradient of fuse_n w.r.t. input i: d / n, or d shared evenly among the inputs equal to the maximum."""
    _f32(d, *[t for t in list(ins) + list(dins) if t is not None])
    if len(ins) != len(dins) or not 1 <= len(ins) <= 8:
        raise _ffi.VltfError("fuse_n_grad: 1..8 inputs and as many gradient slots")
    _ffi.call("vl_fuse_n_grad", _ptr_list(ins), len(ins), _p(d), _ptr_list(dins), d.numel() if count is None else int(count),
              FUSE_OP[method], stream())


# ---- imresize (dataset_.py:481-495) ---------------------------------------------------------------------------------------------
class Resize:
    """scipy.misc.imresize(image, (oh, ow, 3)) = PIL bilinear on uint8 [n, h, w, 3] device images (vl_resize_*), bit-exact."""

    def __init__(self, h, w, oh, ow):
        self.h, self.w, self.oh, self.ow = int(h), int(w), int(oh), int(ow)
        self._d = C.c_void_p()
        _ffi.check(_ffi.lib().vl_resize_create(C.byref(self._d), self.h, self.w, self.oh, self.ow, 3), "vl_resize_create")
        self._tmp = None

    def __del__(self):
        try:
            if self._d:
                _ffi.lib().vl_resize_destroy(self._d)
                self._d = None
        except Exception:
            pass

    def tmp_bytes(self, n):
        """Bytes of the uint8 intermediate of n images (0 when at most one axis changes size)."""
        return int(_ffi.lib().vl_resize_tmp_bytes(self._d, int(n)))

    def __call__(self, src, dst=None, tmp=None):
        """tmp: the caller's intermediate (uint8, >= tmp_bytes(n)); None = this object's own, grown (replaced) on demand -- a captured
        call must own its tmp and dst, which the graph writes on every replay."""
        if src.dtype != torch.uint8 or not src.is_cuda or not src.is_contiguous() or tuple(src.shape[1:]) != (self.h, self.w, 3):
            raise _ffi.VltfError("resize: expected contiguous device uint8 [n, %d, %d, 3], got %s" % (self.h, self.w, tuple(src.shape)))
        n = src.shape[0]
        if dst is None:
            dst = torch.empty((n, self.oh, self.ow, 3), dtype=torch.uint8, device=src.device)
        elif dst.dtype != torch.uint8 or tuple(dst.shape) != (n, self.oh, self.ow, 3) or not dst.is_contiguous():
            raise _ffi.VltfError("resize: destination must be contiguous uint8 %s" % ((n, self.oh, self.ow, 3),))
        need = self.tmp_bytes(n)
        if need and tmp is not None:
            if tmp.dtype != torch.uint8 or not tmp.is_cuda or tmp.numel() < need:
                raise _ffi.VltfError("resize: tmp must be a device uint8 tensor of >= %d bytes" % need)
        elif need:
            if self._tmp is None or self._tmp.numel() < need:
                self._tmp = torch.empty(need, dtype=torch.uint8, device=src.device)
            tmp = self._tmp
        _ffi.call("vl_resize_u8", self._d, _p(src), _p(tmp) if need else None, _p(dst), n, stream())
        return dst
