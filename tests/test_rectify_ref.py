"""CPU: the dense stage of a posed pair as tests/rectify_ref.py states it against the host build of the header the
kernels compile (sfm-gms_amd/csrc/rectify_core.h through tests/cpp/rectify_host.cpp), bit for bit: plans, source positions, bytes
and cloud records; the plan's properties; the cases of tests/rectify_cases.py; and the accuracy of the whole chain on a rendered
plane."""
import ctypes as C

import numpy as np
import pytest

import rectify_cases as rc
import rectify_ref as rr
import hostbuild as hb

SRC = "rectify_host.cpp"
ll = C.c_longlong
VIEW_DTYPE = np.dtype([("R", "<f8", (9,)), ("t", "<f8", (3,)), ("registered", "<i4"), ("pair", "<i4")])


def _camera(camera, dist):
    return np.array(list(camera) + list(dist if dist is not None else (0, 0, 0, 0, 0)), dtype=np.float64)


@pytest.fixture(scope="module")
def host():
    so = hb.host_lib(SRC)
    lib = C.CDLL(so)
    lib.rectify_host_plan.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]
    lib.rectify_host_identity_plan.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p]
    lib.rectify_host_q.argtypes = [C.c_void_p, C.c_void_p]
    lib.rectify_host_positions.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p]
    lib.rectify_host_image.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, ll, C.c_void_p, C.c_int, C.c_int,
                                       ll, C.c_void_p]
    lib.rectify_host_cloud.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int,
                                       C.c_void_p, C.c_void_p]
    return lib


def _host_plan(host, camera, dist, R, t, size, out_size=(0, 0)):
    cam, P = _camera(camera, dist), rr.zero_plan(123)
    R, t = np.ascontiguousarray(R, dtype=np.float64), np.ascontiguousarray(t, dtype=np.float64)
    host.rectify_host_plan(cam.ctypes.data, R.ctypes.data, t.ctypes.data, size[0], size[1], out_size[0], out_size[1], P.ctypes.data)
    return P


def _host_rectify(host, image, camera, dist, plan, which, out_size):
    cam, image = _camera(camera, dist), np.ascontiguousarray(image)
    c = 1 if image.ndim == 2 else 3
    dw, dh = out_size
    dst, valid = np.full((dh, dw) + image.shape[2:], 77, np.uint8), np.full((dh, dw), 77, np.uint8)
    host.rectify_host_image(cam.ctypes.data, plan.ctypes.data, which, image.ctypes.data, image.shape[1], image.shape[0], c, image.shape[1] * c,
                            dst.ctypes.data, dw, dh, dw * c, valid.ctypes.data)
    return dst, valid


# ---- the cases hold what they are named for ---------------------------------------------------------------------------------------------
def test_cases_hold_what_they_are_named_for():
    I = np.eye(3)
    for name in ("t_minus_x", "t_plus_x", "t_minus_y", "t_plus_y", "diagonal_tie", "diagonal_tie_negative"):
        assert np.array_equal(rc.PLAN_CASES[name][1], I)
    t = {k: np.asarray(v[2]) for k, v in rc.PLAN_CASES.items()}
    assert t["t_minus_x"].tolist() == [-1, 0, 0] and t["t_plus_x"].tolist() == [1, 0, 0]
    assert t["t_minus_y"].tolist() == [0, -1, 0] and t["t_plus_y"].tolist() == [0, 1, 0]
    assert abs(t["diagonal_tie"][0]) == abs(t["diagonal_tie"][1]) and abs(t["diagonal_tie_negative"][0]) == abs(t["diagonal_tie_negative"][1])
    for axis, name in enumerate(("rot10_x", "rot10_y", "rot10_z")):
        R = rc.PLAN_CASES[name][1]
        assert abs(np.trace(R) - (1 + 2 * np.cos(np.radians(10)))) < 1e-12 and abs(R[axis, axis] - 1) < 1e-15
    assert abs(t["rot10_z_vertical"][1]) > abs(t["rot10_z_vertical"][0])
    assert np.trace(rc.PLAN_CASES["trace_zero"][1]) <= 0 and np.trace(rc.PLAN_CASES["trace_negative_121"][1]) <= 0
    b = -t["baseline_out_of_plane"]
    assert b[0] > 0 and b[0] < abs(b[2])
    assert t["baseline_along_axis"][0] == 0 and t["baseline_along_axis"][1] == 0
    # the corner (0, 0) of the wide camera, turned by half the pair's rotation either way, is behind one of the two cameras
    fx, fy, cx, cy = rc.CAMERA_WIDE
    corner = np.array([(0 - cx) / fx, (0 - cy) / fy, 1.0])
    assert min((rc.rot((0, 1, 0), a) @ corner)[2] for a in (20, -20)) < 0
    assert np.trace(rc.PLAN_CASES["corner_behind"][1]) > 0 and all(c != 0 for c in rc.DIST_ALL)
    assert set(rc.PLAN_CASES[k][4] for k in rc.OK_PLANS) == {0, 1, 2, 3}


# ---- the statement against the host build -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(rc.PLAN_CASES))
def test_plan_host_build_equals_the_statement_and_the_case(host, name):
    cam, dist, R, t, status, turn = rc.plan_inputs(name)
    for out_size in ((0, 0), (50, 31)):
        want = rr.make_plan(cam, dist, R, t, rc.SIZE_SMALL, out_size)
        got = _host_plan(host, cam, dist, R, t, rc.SIZE_SMALL, out_size)
        assert got.tobytes() == want.tobytes(), (name, got, want)
        assert want["status"][0] == status
        if status == 0:
            assert want["turn"][0] == turn
            W, H = rc.SIZE_SMALL
            assert (want["out_w"][0], want["out_h"][0]) == (out_size if out_size[0] else ((W, H) if turn < 2 else (H, W)))
        else:
            assert want.tobytes() == rr.zero_plan().tobytes()


def test_random_poses_host_build_equals_the_statement(host):
    rng = np.random.default_rng(5)
    n_ok = 0
    for _ in range(200):
        R = rc.rot(rng.normal(size=3), rng.uniform(0, 100))
        t = rng.normal(size=3)
        want = rr.make_plan(rc.CAMERA_SMALL, rc.DIST_ALL, R, t, (67, 45))
        assert _host_plan(host, rc.CAMERA_SMALL, rc.DIST_ALL, R, t, (67, 45)).tobytes() == want.tobytes()
        n_ok += int(want["status"][0] == 0)
    assert 20 < n_ok < 200


@pytest.mark.parametrize("name", rc.OK_PLANS)
def test_plan_properties(name):
    cam, dist, R, t, _, _ = rc.plan_inputs(name)
    P = rr.make_plan(cam, dist, R, t, rc.SIZE_SMALL)[0]
    R1, R2 = P["R1"].reshape(3, 3), P["R2"].reshape(3, 3)
    for M in (R1, R2):
        assert np.abs(M @ M.T - np.eye(3)).max() < 1e-13 and abs(np.linalg.det(M) - 1) < 1e-13
    assert np.abs(R2 @ R @ R1.T - np.eye(3)).max() < 1e-13
    assert np.abs(R2 @ t - np.array([-P["B"], 0, 0])).max() < 1e-13
    assert P["fx"] == P["fy"] == min(cam[0], cam[1]) and P["B"] > 0


def test_q_reprojects_as_the_cloud_does(host):
    cam, dist, R, t, _, _ = rc.plan_inputs("rot10_y")
    P = rr.make_plan(cam, dist, R, t, rc.SIZE_SMALL)
    Q = np.zeros(16)
    host.rectify_host_q(P.ctypes.data, Q.ctypes.data)
    assert Q.tobytes() == rr.plan_q(P).tobytes()
    u, v, d16 = 7, 11, 40
    X = Q.reshape(4, 4) @ np.array([u, v, d16 / 16.0, 1.0])
    disp, valid = np.zeros((29, 37), np.int16), np.ones((29, 37), np.uint8)
    disp[v, u] = d16
    xyz = rr.cloud(disp, valid, None, P, -16)[0][0]
    want = P["R1"][0].reshape(3, 3).T @ (X[:3] / X[3])
    assert np.abs(xyz - want).max() < 1e-5 * np.abs(want).max()


IMAGES = {"37x29": (29, 37), "37x29x3": (29, 37, 3), "67x45x3": (45, 67, 3)}


@pytest.mark.parametrize("shape_name", list(IMAGES))
def test_positions_and_bytes_host_build_equals_the_statement(host, shape_name):
    shape = IMAGES[shape_name]
    im = rc.noise(len(shape_name), *shape)
    size = (shape[1], shape[0])
    camv = _camera(rc.CAMERA_SMALL, rc.DIST_ALL)
    saw_outside = saw_behind = False
    for name in rc.OK_PLANS + ("trace_zero",):
        cam, dist, R, t, _, _ = rc.plan_inputs(name)
        P = rr.make_plan(rc.CAMERA_SMALL, rc.DIST_ALL, R, t, size)
        for which, out_size in ((1, None), (2, (size[0] + 6, size[1] + 3))):
            dw, dh = out_size or (int(P["out_w"][0]) or 9, int(P["out_h"][0]) or 7)
            pos = np.zeros((dh, dw, 5), np.int32)
            host.rectify_host_positions(camv.ctypes.data, P.ctypes.data, which, dw, dh, pos.ctypes.data)
            want = np.stack(rr.source_positions(rc.CAMERA_SMALL, rc.DIST_ALL, P, which, (dw, dh)), axis=-1).astype(np.int32)
            assert np.array_equal(pos, want), (name, which)
            got, gv = _host_rectify(host, im, rc.CAMERA_SMALL, rc.DIST_ALL, P, which, (dw, dh))
            out, valid = rr.rectify(im, rc.CAMERA_SMALL, rc.DIST_ALL, P, which, (dw, dh))
            assert np.array_equal(got, out) and np.array_equal(gv, valid), (name, which)
            saw_outside |= bool((valid == 0).any() and (valid == 1).any())
            if name == "trace_zero":
                assert not out.any() and not valid.any()
    # a ray with z <= 0: a plan made by hand that looks 100 degrees away from the source camera's axis
    P = rr.identity_plan(rc.CAMERA_SMALL, size)
    P["R1"][0] = rc.rot((0, 1, 0), 100).reshape(9)
    out, valid = rr.rectify(im, rc.CAMERA_SMALL, rc.DIST_ALL, P, 1)
    got, gv = _host_rectify(host, im, rc.CAMERA_SMALL, rc.DIST_ALL, P, 1, size)
    front = rr.source_positions(rc.CAMERA_SMALL, rc.DIST_ALL, P, 1, size)[4]
    saw_behind = bool((~front).any())
    assert np.array_equal(got, out) and np.array_equal(gv, valid) and not out[~front].any() and not valid[~front].any()
    assert saw_outside and saw_behind
    # undistort alone
    und = rr.undistort(im, rc.CAMERA_SMALL, rc.DIST_ALL)
    P = rr.identity_plan(rc.CAMERA_SMALL, size)
    hp = rr.zero_plan(99)
    host.rectify_host_identity_plan(camv.ctypes.data, size[0], size[1], hp.ctypes.data)
    assert hp.tobytes() == P.tobytes()
    assert np.array_equal(_host_rectify(host, im, rc.CAMERA_SMALL, rc.DIST_ALL, P, 1, size)[0], und) and not np.array_equal(und, im)


@pytest.mark.parametrize("shape", [(29, 37), (45, 67, 3), (375, 450)])
def test_identity_plan_without_distortion_returns_the_image(shape):
    im = rc.noise(3, *shape)
    cam = (300.0, 310.0, shape[1] / 2.0, shape[0] / 2.0)
    out, valid = rr.rectify(im, cam, None, rr.identity_plan(cam, (shape[1], shape[0])), 1)
    assert np.array_equal(out, im)
    assert valid[:-1, :-1].all() and not valid[-1].any() and not valid[:, -1].any()


def _hand_made_map(seed, h, w, filtered16=-16):
    rng = np.random.default_rng(seed)
    disp = rng.integers(16, 600, (h, w)).astype(np.int16)
    kind = rng.integers(0, 8, (h, w))
    disp[kind == 0] = filtered16
    disp[kind == 1] = 0
    disp[kind == 2] = -rng.integers(1, 300, (h, w)).astype(np.int16)[kind == 2]
    disp[kind == 3] = rng.integers(1, 16, (h, w)).astype(np.int16)[kind == 3]
    valid = (rng.integers(0, 4, (h, w)) != 0).astype(np.uint8) * rng.integers(1, 256, (h, w)).astype(np.uint8)
    return disp, valid


@pytest.mark.parametrize("w,h", [(19, 13), (70, 40)])
def test_cloud_host_build_equals_the_statement(host, w, h):
    disp, valid = _hand_made_map(w, h, w)
    cam, dist, R, t, _, _ = rc.plan_inputs("rot10_x")
    P = rr.make_plan(cam, dist, R, t, (w, h))
    view = np.zeros(1, VIEW_DTYPE)
    view["R"][0], view["t"][0] = rc.rot((1, 2, 3), 25).reshape(9), (0.3, -0.2, 1.5)
    for S, G in ((None, None), (1.75, view)):
        for min16 in (16, 1, 200):
            xyz, _, pixel = rr.cloud(disp, valid, None, P, -16, min16, S, None if G is None else (G["R"][0], G["t"][0]))
            cap = len(xyz) + 5
            gx, gp = np.zeros((cap, 3), np.float32), np.zeros(cap, np.int32)
            Sd = C.c_double(S or 0.0)
            n = host.rectify_host_cloud(disp.ctypes.data, valid.ctypes.data, w, h, P.ctypes.data, -16, min16, C.addressof(Sd),
                                        None if G is None else G.ctypes.data, cap, gx.ctypes.data, gp.ctypes.data)
            assert n == len(xyz) > 0 and gx[:n].tobytes() == xyz.tobytes() and np.array_equal(gp[:n], pixel)
            assert (np.diff(pixel) > 0).all()   # raster order
            d = disp.reshape(-1)[pixel]
            assert (d >= min16).all() and (valid.reshape(-1)[pixel] != 0).all()
            assert n == int(((disp != -16) & (disp >= min16) & (valid != 0)).sum())
    assert rr.cloud(disp, valid, None, rr.zero_plan(), -16)[0].shape == (0, 3)


# ---- accuracy of the chain on a rendered plane ------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def scene_chain():
    return rc.scene_chain()


def test_scene_chain_accuracy(scene_chain):
    P, r1, r2, v1, disp, (xyz, colors, pixel) = scene_chain
    assert P["status"][0] == 0 and P["turn"][0] == 0
    share = rc.scene_depth_error_share(xyz)
    print(f"scene: {len(xyz)} points, share within 1 px of disparity {share:.4f}, valid share {v1.mean():.3f}")
    assert len(xyz) > 3000
    assert abs(share - rc.SCENE_SHARE_MEASURED) < 5e-4          # the recorded figure is this chain's
    assert share >= rc.SCENE_SHARE_MEASURED - rc.SCENE_SHARE_MARGIN
    assert np.array_equal(colors, r1.reshape(-1)[pixel])


def test_stand_alone_program_under_sanitizers():
    exe = hb.host_exe_sanitized(SRC, defines=("RECTIFY_HOST_MAIN",))
    out = hb.run(exe)
    assert out.returncode == 0, out.stderr
    assert out.stdout.startswith("rectify_host: checksum ")
