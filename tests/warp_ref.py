"""cv::resize (INTER_LINEAR) and cv::warpAffine (INTER_LINEAR, BORDER_CONSTANT 0) for 8-bit images of 1 or 3 interleaved channels,
and getRotationMatrix2D / img_rotate, stated in numpy. This is the definition the library is held to byte for
byte: csrc/warp_core.h says the same in C++ for the kernels and the host build. The statement is read from OpenCV 4.5.2's published
source; parity with an OpenCV build is unpinned."""
import math

import numpy as np


def _round_short(v):
    """saturate_cast<short>(float): round half to even, then clamp."""
    return np.clip(np.rint(v), -32768, 32767).astype(np.int64)


def _round_i32(v):
    return np.clip(np.rint(v), -2.0 ** 31, 2.0 ** 31 - 1).astype(np.int64)


def axis_scale(dn, sn):
    return np.float64(1.0) / (np.float64(dn) / np.float64(sn))


def _axis(dn, sn):
    """-> (first source index, fraction as float32) per destination index, before any clamping."""
    d = np.arange(dn, dtype=np.float64)
    f = ((d + 0.5) * axis_scale(dn, sn) - 0.5).astype(np.float32)
    s = np.floor(f).astype(np.int64)
    return s, (f - s.astype(np.float32)).astype(np.float32)


def resize(src, dsize):
    """src uint8 [H, W] or [H, W, C]; dsize = (width, height), as cv::resize takes it."""
    dw, dh = int(dsize[0]), int(dsize[1])
    src = np.asarray(src, dtype=np.uint8)
    sh, sw = src.shape[:2]
    im = src.reshape(sh, sw, -1).astype(np.int64)
    shape = (dh, dw) + src.shape[2:]
    if axis_scale(dw, sw) == 2.0 and axis_scale(dh, sh) == 2.0:
        o = (im[0::2, 0::2] + im[0::2, 1::2] + im[1::2, 0::2] + im[1::2, 1::2] + 2) >> 2
        return o.astype(np.uint8).reshape(shape)
    sx, fx = _axis(dw, sw)
    sy, fy = _axis(dh, sh)
    lo = sx < 0
    sx, fx = np.where(lo, 0, sx), np.where(lo, np.float32(0), fx)
    hi = sx >= sw - 1
    sx, fx = np.where(hi, sw - 1, sx), np.where(hi, np.float32(0), fx)
    a0 = _round_short((np.float32(1) - fx) * np.float32(2048))
    a1 = _round_short(fx * np.float32(2048))
    sx1 = np.minimum(sx + 1, sw - 1)   # (weight 0 wherever it was clamped)
    H = im[:, sx] * a0[None, :, None] + im[:, sx1] * a1[None, :, None]
    b0 = _round_short((np.float32(1) - fy) * np.float32(2048))
    b1 = _round_short(fy * np.float32(2048))
    r0, r1 = np.clip(sy, 0, sh - 1), np.clip(sy + 1, 0, sh - 1)
    o = (((b0[:, None, None] * (H[r0] >> 4)) >> 16) + ((b1[:, None, None] * (H[r1] >> 4)) >> 16) + 2) >> 2
    return o.astype(np.uint8).reshape(shape)


def getRotationMatrix2D(center, angle, scale):
    cx, cy = float(np.float32(center[0])), float(np.float32(center[1]))
    a = angle * math.pi / 180
    al, be = math.cos(a) * scale, math.sin(a) * scale
    return np.array([[al, be, (1 - al) * cx - be * cy], [-be, al, be * cx + (1 - al) * cy]], dtype=np.float64)


def invert_affine(M):
    F = np.asarray(M, dtype=np.float64).reshape(6)
    D = F[0] * F[4] - F[1] * F[3]
    D = 1.0 / D if D != 0 else 0.0
    m = np.zeros(6)
    m[0], m[4] = F[4] * D, F[0] * D
    m[1], m[3] = F[1] * (-D), F[3] * (-D)
    m[2] = -m[0] * F[2] - m[1] * F[5]
    m[5] = -m[3] * F[2] - m[4] * F[5]
    return m


def warpAffine(src, M, dsize):
    """src uint8 [H, W] or [H, W, C]; M the forward 2 x 3 matrix; dsize = (width, height)."""
    dw, dh = int(dsize[0]), int(dsize[1])
    src = np.asarray(src, dtype=np.uint8)
    sh, sw = src.shape[:2]
    im = src.reshape(sh, sw, -1).astype(np.int64)
    m = invert_affine(M)
    x, y = np.arange(dw, dtype=np.float64), np.arange(dh, dtype=np.float64)
    ad, bd = _round_i32(m[0] * x * 1024), _round_i32(m[3] * x * 1024)
    X0, Y0 = _round_i32((m[1] * y + m[2]) * 1024) + 16, _round_i32((m[4] * y + m[5]) * 1024) + 16
    X, Y = (X0[:, None] + ad[None, :]) >> 5, (Y0[:, None] + bd[None, :]) >> 5
    ix, iy = np.clip(X >> 5, -32768, 32767), np.clip(Y >> 5, -32768, 32767)
    fx, fy = (X & 31)[..., None], (Y & 31)[..., None]

    def tap(yy, xx):
        ok = (xx >= 0) & (xx < sw) & (yy >= 0) & (yy < sh)
        return np.where(ok[..., None], im[np.clip(yy, 0, sh - 1), np.clip(xx, 0, sw - 1)], 0)

    S = (tap(iy, ix) * (32 - fx) * (32 - fy) + tap(iy, ix + 1) * fx * (32 - fy) + tap(iy + 1, ix) * (32 - fx) * fy
         + tap(iy + 1, ix + 1) * fx * fy)
    return ((S + 512) >> 10).astype(np.uint8).reshape((dh, dw) + src.shape[2:])


def img_rotate(src, angle):
    """The reference's img_rotate (main.cpp:114-120): about (w / 2., h / 2.), scale 1, same size."""
    h, w = np.asarray(src).shape[:2]
    return warpAffine(src, getRotationMatrix2D((w / 2., h / 2.), angle, 1.0), (w, h))
