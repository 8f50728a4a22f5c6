"""What the GPU tests of LOGOS share (tests/test_gpu_logos.py, test_gpu_logos_batch.py, test_gpu_logos_limits.py): keypoint and DMatch
records from plain arrays, the one-shot with its result record, and the batched filter on a canary-filled output."""
import ctypes as C
import importlib

import numpy as np

pkg = importlib.import_module("sfm-gms_amd")
GMS_ERR_BAD_ARG, GMS_ERR_DOMAIN, GMS_ERR_CAPACITY = -1, -2, -5


def kp_records(a4):
    a4 = np.asarray(a4, np.float32).reshape(-1, 4)
    k = np.zeros(len(a4), pkg.KEYPOINT_DTYPE)
    k["x"], k["y"], k["size"], k["angle"] = a4[:, 0], a4[:, 1], a4[:, 2], a4[:, 3]
    k["class_id"] = -1
    return k


def want_dmatch(pairs):
    pairs = np.asarray(pairs).reshape(-1, 2)
    out = np.zeros(len(pairs), pkg.DMATCH_DTYPE)
    out["queryIdx"], out["trainIdx"], out["imgIdx"] = pairs[:, 0], pairs[:, 1], -1
    return out


def oneshot(kp1, kp2, l1, l2):
    """gms_logos_match with room for everything: (survivors, LOGOS_RESULT_DTYPE record)."""
    lib = pkg.load_library()
    l1 = np.ascontiguousarray(l1, np.int32)
    l2 = np.ascontiguousarray(l2, np.int32)
    cap = max(len(kp1), len(kp2), 1)
    for _ in range(2):
        out = np.zeros(cap, pkg.DMATCH_DTYPE)
        n = C.c_int64(0)
        res = np.zeros(1, pkg.LOGOS_RESULT_DTYPE)
        rc = lib.gms_logos_match(kp1.ctypes.data, len(kp1), kp2.ctypes.data, len(kp2), l1.ctypes.data, l2.ctypes.data, out.ctypes.data,
                                 cap, C.byref(n), res.ctypes.data)
        if rc != GMS_ERR_CAPACITY:
            break
        cap = n.value
    assert rc == 0
    return out[: n.value].copy(), res[0]


def device_run(ctx, table, pairs, prefill=0x5A, extra=0, ws_fill=None, ws_bytes=None):
    """gms_logos_filter_device with d_out prefilled (canaries), `extra` spare records past the last range, the workspace filled
    with ws_fill if given (what a reused workspace may hold), of ws_bytes if given (default: what the batch needs)."""
    import torch
    batch = importlib.import_module("sfm-gms_amd.batch")
    dev = table.device
    n = len(pairs)
    total = int((pairs["match_off"] + pairs["m"]).max()) + extra
    max_q = int(table.counts[pairs["frame_a"][(pairs["frame_a"] >= 0) & (pairs["frame_a"] < table.n_frames)]].max())
    ws = ctx.logos_workspace_bytes(0, n, max_q) if ws_bytes is None else int(ws_bytes)
    d_pairs = batch._to_dev(pairs, dev)
    d_ws = (torch.empty(max(ws, 16), dtype=torch.uint8, device=dev) if ws_fill is None else
            torch.full((max(ws, 16),), ws_fill, dtype=torch.uint8, device=dev))
    d_out = torch.full((max(total, 1) * 16,), prefill, dtype=torch.uint8, device=dev)
    d_lres = torch.zeros(n * 32, dtype=torch.uint8, device=dev)
    d_pres = torch.zeros(n * 16, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize(dev)
    table.filter_device(d_pairs.data_ptr(), n, d_ws.data_ptr(), ws, d_out.data_ptr(), d_lres.data_ptr(), d_pres.data_ptr())
    ctx.synchronize()
    return (d_out.cpu().numpy(), d_lres.cpu().numpy().view(pkg.LOGOS_RESULT_DTYPE), d_pres.cpu().numpy().view(pkg.RESULT_DTYPE))
