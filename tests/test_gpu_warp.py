"""GPU: gms_resize_device / gms_warp_affine_device and their Python faces against tests/warp_ref.py, byte for byte,
at the smallest shapes at which the kernels can go wrong: one pixel, rows shorter than a lane's four bytes, byte tails and unaligned
pitched rows, tiles crossed in both axes, every resize path, taps that leave the source on every side; one graph capture replayed on
new matrices; the refused arguments."""
import importlib

import numpy as np
import pytest

import warp_ref

pytestmark = pytest.mark.gpu


def _noise(seed, *shape):
    return np.random.default_rng(seed).integers(0, 256, shape, dtype=np.uint8)


@pytest.fixture(scope="module")
def batch():
    return importlib.import_module("sfm-gms_amd.batch")


@pytest.mark.parametrize("shape,dsizes", [
    ((1, 1), [(1, 1), (3, 2), (300, 20)]),
    ((5, 2), [(2, 5), (1, 1), (5, 2), (9, 9), (1, 2)]),                    # 2 wide, 5 high
    ((17, 23), [(130, 70)]),                                              # upscale across a tile edge in both axes
    ((375, 450), [(100, 90)]),                                            # shrink by more than 2
    ((375, 450, 3), [(100, 90), (300, 200)]),
    ((46, 74), [(37, 23), (37, 46), (74, 23)]),                           # the exact 2 x 2 mean; 2 x in one axis alone
    ((46, 74, 3), [(37, 23), (37, 46)]),
    ((40, 1040), [(520, 20)]),                                            # the 2 x 2 mean past one tile of one-channel dwords
])
def test_resize_equals_the_statement(pkg, shape, dsizes):
    im = _noise(sum(shape), *shape)
    for dsize in dsizes:
        got = pkg.resize(im, dsize)
        assert got.shape == (dsize[1], dsize[0]) + im.shape[2:]
        assert np.array_equal(got, warp_ref.resize(im, dsize)), dsize


def _pitched(torch, imgs, pitch, fill):
    """The images [n, H, W, C] in a device buffer whose rows are `pitch` bytes apart, the gaps holding `fill`."""
    n, h = imgs.shape[:2]
    row = imgs.reshape(n, h, -1)
    buf = np.full((n, h, pitch), fill, np.uint8)
    buf[:, :, :row.shape[2]] = row
    return torch.from_numpy(buf).cuda()


@pytest.mark.parametrize("w", [37, 67])
def test_pitched_unaligned_rows_and_untouched_gaps(ctx, w):
    import torch
    n, h, dw, dh = 2, 19, w + 6, 21
    imgs = _noise(w, n, h, w, 3)
    sp, dp = 3 * w + 5, 3 * dw + 5
    d_src = _pitched(torch, imgs, sp, 7)
    M = np.stack([warp_ref.getRotationMatrix2D((w / 2., h / 2.), 30, 1.0), warp_ref.getRotationMatrix2D((5, 5), -75, 0.6)]).reshape(2, 6)
    d_M = torch.from_numpy(M).cuda()
    for what in ("resize", "halve", "warp"):
        ow, oh = (dw, dh) if what != "halve" else (w // 2, h // 2)
        sw_, sh_ = (w, h) if what != "halve" else (2 * (w // 2), 2 * (h // 2))   # the even part of the image, same pitch
        op = 3 * ow + 5
        d_dst = torch.full((n, oh, op), 0xA5, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        if what == "warp":
            ctx.warp_affine_device(d_src.data_ptr(), n, w, h, 3, sp, d_M.data_ptr(), 2, d_dst.data_ptr(), ow, oh, op)
        elif what == "resize":
            ctx.resize_device(d_src.data_ptr(), n, w, h, 3, sp, d_dst.data_ptr(), ow, oh, op)
        else:
            # image i still starts at i * h * sp: one image at a time, so that the shorter height does not move the second one
            for i in range(n):
                ctx.resize_device(d_src[i].data_ptr(), 1, sw_, sh_, 3, sp, d_dst[i].data_ptr(), ow, oh, op)
        ctx.synchronize()
        got = d_dst.cpu().numpy()
        assert (got[:, :, 3 * ow:] == 0xA5).all(), what
        for i in range(n):
            src = imgs[i, :sh_, :sw_]
            want = warp_ref.warpAffine(src, M[i], (ow, oh)) if what == "warp" else warp_ref.resize(src, (ow, oh))
            assert np.array_equal(got[i, :, :3 * ow].reshape(oh, ow, 3), want), (what, i)


def test_warp_affine_three_images_three_matrices(batch):
    """30 degrees, -75 degrees at scale 0.6 and a translation by (-40.25, 300): the taps cross all four borders and, for the
    translation, leave the source entirely (300 > its height); destination size != source size."""
    w, h = 211, 120
    imgs = _noise(9, 3, h, w, 3)
    M = np.stack([warp_ref.getRotationMatrix2D((w / 2., h / 2.), 30, 1.0), warp_ref.getRotationMatrix2D((60.5, 100.25), -75, 0.6),
                  np.array([[1, 0, -40.25], [0, 1, 300.0]])])
    for dsize in [(w, h), (300, 77)]:
        got = batch.warp_affine_images(imgs, M, dsize)
        want = [warp_ref.warpAffine(imgs[i], M[i], dsize) for i in range(3)]
        for i in range(3):
            assert np.array_equal(got[i], want[i]), (dsize, i)
        assert want[0].any() and (want[0] == 0).any() and not want[2].any()
    grey = np.ascontiguousarray(imgs[:, :, :, 0])
    got = batch.warp_affine_images(grey, M, (w + 3, h + 2))
    for i in range(3):
        assert np.array_equal(got[i], warp_ref.warpAffine(grey[i], M[i], (w + 3, h + 2)))


def test_one_matrix_for_all_images_identity_and_singular(batch):
    imgs = _noise(11, 3, 23, 37, 3)
    eye = np.array([[1., 0, 0], [0, 1, 0]])
    assert np.array_equal(batch.warp_affine_images(imgs, eye, (37, 23)), imgs)
    sing = np.array([[1., 2, 3], [2, 4, 5]])
    got = batch.warp_affine_images(imgs, sing, (11, 9))
    assert np.array_equal(got, np.broadcast_to(imgs[:, :1, :1], (3, 9, 11, 3)))
    rot = warp_ref.getRotationMatrix2D((10, 7), 40, 1.3)
    got = batch.warp_affine_images(imgs, rot, (50, 30))
    for i in range(3):
        assert np.array_equal(got[i], warp_ref.warpAffine(imgs[i], rot, (50, 30)))


@pytest.mark.parametrize("shape", [(1, 1), (5, 2), (23, 37, 3), (375, 450, 3)])
def test_img_rotate_and_tiny_images(pkg, shape):
    im = _noise(13, *shape)
    h, w = shape[:2]
    for angle in (180, 90, 30):
        assert np.array_equal(pkg.imgRotate(im, angle), warp_ref.img_rotate(im, angle)), angle
    M = warp_ref.getRotationMatrix2D((0.5, 0.25), 10, 0.5)
    assert np.array_equal(pkg.warpAffine(im, M, (w + 4, h + 1)), warp_ref.warpAffine(im, M, (w + 4, h + 1)))
    assert pkg.getRotationMatrix2D((w / 2., h / 2.), 30, 1.0).tobytes() == warp_ref.getRotationMatrix2D((w / 2., h / 2.), 30, 1.0).tobytes()


def test_rotation_by_180_of_a_1080p_image_is_the_shifted_flip(pkg):
    im = _noise(15, 1080, 1920)
    got = pkg.imgRotate(im, 180)
    assert np.array_equal(got[1:, 1:], im[::-1, ::-1][:-1, :-1]) and not got[0].any() and not got[:, 0].any()


def test_device_tensors_in_device_tensors_out(pkg, batch):
    import torch
    im = _noise(17, 23, 37, 3)
    d = torch.from_numpy(im).cuda()
    out = pkg.resize(d, (50, 9))
    assert torch.is_tensor(out) and out.is_cuda and np.array_equal(out.cpu().numpy(), warp_ref.resize(im, (50, 9)))
    out = pkg.imgRotate(d, 180)
    assert torch.is_tensor(out) and np.array_equal(out.cpu().numpy(), warp_ref.img_rotate(im, 180))
    out = batch.resize_images(torch.stack([d, d]), (18, 11))
    assert out.shape == (2, 11, 18, 3) and np.array_equal(out[1].cpu().numpy(), warp_ref.resize(im, (18, 11)))


def test_capture_and_replay_follows_new_matrices(ctx, batch):
    import torch
    n, w, h = 2, 67, 41
    imgs = _noise(19, n, h, w, 3)
    d = torch.from_numpy(imgs).cuda()
    run = batch.Warp(ctx, n, (w, h), (80, 50), channels=3, n_matrices=n)
    sets = [np.stack([warp_ref.getRotationMatrix2D((w / 2., h / 2.), a, s), warp_ref.getRotationMatrix2D((10, 30), -a, 1.0)])
            for a, s in ((30, 1.0), (180, 1.0), (-75, 0.6))]
    run.set_matrices(sets[0])
    torch.cuda.synchronize()
    run.warp_affine(d)
    ctx.synchronize()
    stream = torch.cuda.Stream()
    ctx.set_stream(stream.cuda_stream)
    try:
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=stream):
            run.warp_affine(d)
        for M in sets[1:] + sets[:1]:
            run.set_matrices(M)
            run.d_dst.zero_()
            torch.cuda.synchronize()
            g.replay()
            torch.cuda.synchronize()
            got = run.d_dst.cpu().numpy()
            for i in range(n):
                assert np.array_equal(got[i], warp_ref.warpAffine(imgs[i], M[i], (80, 50)))
    finally:
        ctx.set_stream(None)


def test_bad_arguments_rejected_and_nothing_written(ctx, pkg):
    import torch
    types = importlib.import_module("sfm-gms_amd.types")
    w, h = 16, 8
    d_src = torch.zeros(4 * h * w * 3, dtype=torch.uint8, device="cuda")
    d_dst = torch.full((4 * h * w * 3,), 0xA5, dtype=torch.uint8, device="cuda")
    d_M = torch.tensor([[1., 0, 0, 0, 1, 0]], dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    s, o, m = d_src.data_ptr(), d_dst.data_ptr(), d_M.data_ptr()
    bad = [
        dict(channels=2), dict(channels=4), dict(sw=0), dict(sh=0), dict(dw=0), dict(dh=0), dict(sw=8193), dict(dh=8193), dict(n=0),
        dict(n=65536), dict(sp=3 * w - 1), dict(dp=3 * w - 1), dict(dst=s), dict(dst=s + 5), dict(dst=s + 3 * w * h - 1), dict(src=None),
    ]
    for kw in bad:
        a = dict(src=s, n=1, sw=w, sh=h, channels=3, sp=3 * w, dst=o, dw=w, dh=h, dp=3 * w)
        a.update(kw)
        with pytest.raises(types.GmsError) as e:
            ctx.resize_device(a["src"], a["n"], a["sw"], a["sh"], a["channels"], a["sp"], a["dst"], a["dw"], a["dh"], a["dp"])
        assert e.value.code == -1, kw
        with pytest.raises(types.GmsError) as e:
            ctx.warp_affine_device(a["src"], a["n"], a["sw"], a["sh"], a["channels"], a["sp"], m, 1, a["dst"], a["dw"], a["dh"], a["dp"])
        assert e.value.code == -1, kw
    for n_matrices, d_m in ((2, m), (0, m), (1, None)):
        with pytest.raises(types.GmsError) as e:
            ctx.warp_affine_device(s, 3, w, h, 3, 3 * w, d_m, n_matrices, o, w, h, 3 * w)
        assert e.value.code == -1
    ctx.synchronize()
    assert (d_dst.cpu().numpy() == 0xA5).all()
    im = np.zeros((h, w, 2), np.uint8)
    for call in (lambda: pkg.resize(im, (4, 4)), lambda: pkg.resize(np.zeros((h, w), np.uint8), (0, 4)),
                 lambda: pkg.warpAffine(np.zeros((h, w), np.uint8), np.eye(3), (4, 4))):
        with pytest.raises((ValueError, types.GmsError)):
            call()
