"""Host-side mirror of util::stereo_rectifier and util::image_converter (expected: src/openvslam/util/stereo_rectifier.h, image_converter.h)
over the C ABI: gray conversion and stereo rectification by one kernel launch. The computation is the HIP library's."""
import ctypes as C

import numpy as np

from . import _lib

GRAY, RGB, BGR = 0, 1, 2                # upstream's color_order_t
COLOR_ORDERS = {"gray": GRAY, "rgb": RGB, "bgr": BGR, GRAY: GRAY, RGB: RGB, BGR: BGR}
MODELS = {"perspective": 0, "fisheye": 1, 0: 0, 1: 1}


def _p(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


def rectify_side(side):
    """dict(model, K (3x3), D (0, 4, 5 or 8 coefficients; n_dist overrides their count), R (3x3)) -> ovs_rectify_side."""
    D = [float(v) for v in np.asarray(side.get("D", []), np.float64).ravel()]
    if len(D) > 8:
        raise ValueError("at most 8 distortion coefficients")
    s = _lib.RectifySide()
    s.model = MODELS[side.get("model", 0)]
    s.n_dist = int(side.get("n_dist", len(D)))
    s.K[:] = [float(v) for v in np.asarray(side["K"], np.float64).ravel()]
    s.D[:] = D + [0.0] * (8 - len(D))
    s.R[:] = [float(v) for v in np.asarray(side.get("R", np.eye(3)), np.float64).ravel()]
    return s


def _image(img):
    """(array, rows, cols, channels, row stride) of an 8-bit image of 1, 3 or 4 channels; rows keep their stride, pixels are made dense."""
    img = np.asarray(img)
    if img.dtype != np.uint8 or img.ndim not in (2, 3):
        raise TypeError("image must be 8-bit, (rows, cols) or (rows, cols, channels)")
    channels = 1 if img.ndim == 2 else img.shape[2]
    if img.size and not (img.strides[-1] == 1 and (img.ndim == 2 or img.strides[1] == channels) and img.strides[0] >= img.shape[1] * channels):
        img = np.ascontiguousarray(img)
    return img, img.shape[0], img.shape[1], channels, (img.strides[0] if img.size else 0)


class image_preparer:
    """The handle (ovs_imgprep): device planes for images of up to max_rows x max_cols and the resident maps of one rig."""

    def __init__(self, max_rows=1080, max_cols=1920, device=0):
        self._L = _lib.lib()
        self._h = None
        h = C.c_void_p()
        _lib.check(self._L.ovs_imgprep_create(device, max_rows, max_cols, C.byref(h)), "ovs_imgprep_create")
        self._h = h
        self.map_shape = None

    def __del__(self):
        if getattr(self, "_h", None):
            self._L.ovs_imgprep_destroy(self._h)
            self._h = None

    def set_rectifier(self, rows, cols, left, right, rect_camera):
        """Builds and uploads the fixed-point maps of a rig. left / right: dicts for rectify_side (right may be None); rect_camera: fx, fy, cx, cy."""
        sl, sr = rectify_side(left), rectify_side(right) if right is not None else None
        P = (C.c_double * 4)(*[float(v) for v in rect_camera])
        _lib.check(self._L.ovs_imgprep_set_rectifier(self._h, rows, cols, C.byref(sl), C.byref(sr) if sr is not None else None, P), "ovs_imgprep_set_rectifier")
        self.map_shape = (rows, cols)

    def set_maps(self, map_x_left, map_y_left, map_x_right=None, map_y_right=None):
        """The caller's own float32 maps (e.g. cv2.initUndistortRectifyMap's), converted to the resident fixed-point form."""
        maps = [None if m is None else np.ascontiguousarray(m, np.float32) for m in (map_x_left, map_y_left, map_x_right, map_y_right)]
        rows, cols = maps[0].shape
        if any(m is not None and m.shape != (rows, cols) for m in maps):
            raise ValueError("maps must have one size")
        _lib.check(self._L.ovs_imgprep_set_maps(self._h, rows, cols, *[_p(m) for m in maps]), "ovs_imgprep_set_maps")
        self.map_shape = (rows, cols)

    def get_maps(self, side=0):
        """The resident map of a side, read back: ixy (rows, cols, 2) int16 and fxy (rows, cols, 2) uint8."""
        if self.map_shape is None:
            raise _lib.OvsError(-1, "ovs_imgprep_get_maps")
        ixy, fxy = np.zeros(self.map_shape + (2,), np.int16), np.zeros(self.map_shape + (2,), np.uint8)
        _lib.check(self._L.ovs_imgprep_get_maps(self._h, side, _p(ixy), _p(fxy)), "ovs_imgprep_get_maps")
        return ixy, fxy

    def run(self, left, right=None, color_order=GRAY, rectify=False):
        """The prepared (gray, rectified if asked) image, or the pair of them."""
        l, rows, cols, ch, stride = _image(left)
        out_l = np.zeros((rows, cols), np.uint8)
        r = out_r = None
        if right is not None:
            r, rows_r, cols_r, ch_r, stride_r = _image(right)
            if (rows_r, cols_r, ch_r) != (rows, cols, ch):
                raise ValueError("both images must have one size and channel count")
            if stride_r != stride:
                l, r = np.ascontiguousarray(l), np.ascontiguousarray(r)
                stride = cols * ch
            out_r = np.zeros((rows, cols), np.uint8)
        _lib.check(self._L.ovs_imgprep_run(self._h, _p(l), _p(r), rows, cols, stride, ch, COLOR_ORDERS[color_order], 1 if rectify else 0, _p(out_l), _p(out_r),
                                           cols), "ovs_imgprep_run")
        return out_l if right is None else (out_l, out_r)

    def run_dev(self, d_left, d_right, channels, color_order, rectify, d_out_left, d_out_right, stream=None):
        """Device form on torch uint8 CUDA tensors: sources (rows, cols * channels), outputs (rows, cols); row strides are the tensors'. Asynchronous."""
        rows, cols = d_out_left.shape
        _lib.check(self._L.ovs_imgprep_run_dev(self._h, d_left.data_ptr(), d_right.data_ptr() if d_right is not None else None, rows, cols, d_left.stride(0),
                                               channels, COLOR_ORDERS[color_order], 1 if rectify else 0, d_out_left.data_ptr(),
                                               d_out_right.data_ptr() if d_out_right is not None else None, d_out_left.stride(0), stream), "ovs_imgprep_run_dev")


class stereo_rectifier:
    """util::stereo_rectifier. cfg keys: model ("perspective" | "fisheye"), K_left, D_left, R_left, K_right, D_right, R_right, and the rectified
    camera as fx, fy, cx, cy, cols, rows (upstream: the camera the rectifier is constructed with)."""

    def __init__(self, cfg, device=0, preparer=None):
        self.rows, self.cols = int(cfg["rows"]), int(cfg["cols"])
        self.preparer = preparer or image_preparer(self.rows, self.cols, device)
        model = cfg.get("model", "perspective")
        sides = [dict(model=model, K=cfg["K_" + s], D=cfg["D_" + s], R=cfg["R_" + s]) for s in ("left", "right")]
        self.preparer.set_rectifier(self.rows, self.cols, sides[0], sides[1], [cfg[k] for k in ("fx", "fy", "cx", "cy")])

    def rectify(self, in_img_l, in_img_r):
        """(out_img_l, out_img_r): every channel remapped. A colour image stays a colour image, as upstream's does."""
        outs = []
        l, r = np.asarray(in_img_l), np.asarray(in_img_r)
        if l.ndim == 2:
            return self.preparer.run(l, r, GRAY, True)
        for c in range(l.shape[2]):   # the channels are independent (rule I2): one gray pass each
            outs.append(self.preparer.run(np.ascontiguousarray(l[..., c]), np.ascontiguousarray(r[..., c]), GRAY, True))
        return np.stack([o[0] for o in outs], -1), np.stack([o[1] for o in outs], -1)


def convert_to_grayscale(img, color_order, preparer=None, device=0):
    """util::convert_to_grayscale: the gray image of an 8-bit image of 1, 3 or 4 channels."""
    img = np.asarray(img)
    p = preparer or image_preparer(max(1, img.shape[0]), max(1, img.shape[1]), device)
    return p.run(img, None, color_order, False)
