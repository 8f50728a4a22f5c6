"""Device-resident batch driver: resident frame tables + pair descriptors -> filtered matches.

torch is used here for what the project allows it for: device memory and streams. The filter itself
is gms_filter_device in csrc/libgms_hip.so. Mirrors how the reference's callers use matchGMS
(FeatureMatchUtil.cpp:66-69: M = N1 matches from BFMatcher, then one matchGMS per image pair), but
for many pairs per launch with the per-frame keypoint tables kept in HBM.
"""
import numpy as np
import torch

from .api import GmsContext, logos_dict_args
from .types import (BF_RESULT_DTYPE, DMATCH_DTYPE, GMS_DESC_HAMMING256, GMS_DESC_L2_F32X128, GMS_ERR_CAPACITY, KEYPOINT_DTYPE, LOGOS_DICT_RESULT_DTYPE, LOGOS_RESULT_DTYPE, PAIR_DTYPE,
                    RESULT_DTYPE, concat_frames, desc_layout, portrait_params, stereo_bm_params, stereo_sgm_params, CAMERA_DTYPE, GMS_ERR_BAD_ARG, GmsError,
                    RECTIFY_PLAN_DTYPE, TWO_VIEW_DTYPE, make_camera, rectify_plan_records, DENSE_FUSE_SRC_DTYPE, dense_fuse_neighbors, SFM_VIEW_DTYPE,
                    SFM_PAIR_REG_DTYPE)


def _to_dev(arr, device):
    a = np.ascontiguousarray(arr)
    return torch.from_numpy(a.view(np.uint8).reshape(-1)).to(device)


def _device(ctx, device):
    return torch.device(device if device is not None else f"cuda:{ctx.device}")


def frame_counts(counts, idx):
    """counts[idx] for every frame index of idx; 0 for an index out of range, also when there are no frames."""
    counts, idx = np.asarray(counts, dtype=np.int64), np.asarray(idx, dtype=np.int64)
    return np.append(counts, 0)[np.where((idx >= 0) & (idx < len(counts)), idx, len(counts))]


def pair_table(frame_pairs, capacity):
    """PAIR_DTYPE records for (frame_a, frame_b) pairs: m = capacity (an int or one per pair), match_off = the running sum of the
    max(m, 0) before each pair, so that the pairs' ranges lie back to back."""
    fp = np.asarray(frame_pairs, dtype=np.int64).reshape(-1, 2)
    recs = np.zeros(len(fp), PAIR_DTYPE)
    cap = np.broadcast_to(np.asarray(capacity, dtype=np.int64), (len(fp),))
    room = np.maximum(cap, 0)
    recs["frame_a"], recs["frame_b"], recs["m"], recs["match_off"] = fp[:, 0], fp[:, 1], cap, np.cumsum(room) - room
    return recs


def frame_pairs_of(recs):
    """The (frame_a, frame_b) columns of PAIR_DTYPE records, as pair_table takes them."""
    return np.stack([recs["frame_a"], recs["frame_b"]], axis=1)


def _survivors(out, recs, res):
    return [out[o:o + (k if st == 0 else 0)].copy()
            for o, k, st in zip(recs["match_off"].tolist(), res["n_out"].tolist(), res["status"].tolist())]


def run_with_retry(recs, run):
    """run(PAIR_DTYPE records) -> (output laid out by match_off, result records with n_out and status). Pairs that come back with
    GMS_ERR_CAPACITY are run once more, together, with the count they reported as their room: (list of per-pair survivor arrays,
    result records with those of the second run merged in). A pair whose status is not 0 in the end has no survivors."""
    out, res = run(recs)
    got = _survivors(out, recs, res)
    over = np.nonzero(res["status"] == GMS_ERR_CAPACITY)[0]
    if len(over):
        again = pair_table(frame_pairs_of(recs[over]), res["n_out"][over])
        out2, res[over] = run(again)
        for p, kept in zip(over, _survivors(out2, again, res[over])):
            got[p] = kept
    return got, res


class FrameTable:
    """Keypoints of all frames of a sequence, normalised once on the GPU (GMSMatcher::normalizePoints)."""

    def __init__(self, ctx, keypoints_per_frame, sizes, device="cuda:0"):
        self.ctx = ctx
        self.device = torch.device(device)
        self.n_frames = len(keypoints_per_frame)
        kp_all, self.frame_off_host = concat_frames(keypoints_per_frame)
        self.total = int(self.frame_off_host[-1])
        wh = np.asarray(sizes, dtype=np.int32).reshape(-1, 2)
        assert wh.shape[0] == self.n_frames
        self.d_kp = _to_dev(kp_all, self.device)
        self.d_frame_off = torch.from_numpy(self.frame_off_host).to(self.device)
        self.d_wh = torch.from_numpy(wh.reshape(-1).copy()).to(self.device)
        # the frame table: normalised points, then the per-keypoint cell codes (gms_frame_table_bytes)
        self.d_pts = torch.zeros(ctx.frame_table_bytes(self.total) // 4, dtype=torch.float32, device=self.device)
        torch.cuda.synchronize(self.device)
        ctx.normalize_device(self.d_kp.data_ptr(), self.d_frame_off.data_ptr(), self.d_wh.data_ptr(),
                             self.n_frames, self.total, self.d_pts.data_ptr())
        ctx.synchronize()

    @classmethod
    def from_device(cls, ctx, d_kp, d_frame_off, sizes):
        """The table of keypoints that are on the device already: d_kp a tensor of KEYPOINT_DTYPE records, all frames back to back,
        d_frame_off int64 [n_frames + 1] (what gms_detect_pack_device leaves). The offsets are read back -- the one readback: they size
        d_pts and are frame_off_host -- the keypoints are not. Waits for the context's stream first (the offsets come from it)."""
        self = cls.__new__(cls)
        self.ctx, self.device = ctx, d_kp.device
        ctx.synchronize()
        self.frame_off_host = d_frame_off.cpu().numpy().astype(np.int64)
        self.n_frames, self.total = len(self.frame_off_host) - 1, int(self.frame_off_host[-1])
        wh = np.asarray(sizes, dtype=np.int32).reshape(-1, 2)
        assert wh.shape[0] == self.n_frames
        self.d_kp, self.d_frame_off = d_kp, d_frame_off
        self.d_wh = torch.from_numpy(wh.reshape(-1).copy()).to(self.device)
        self.d_pts = torch.zeros(ctx.frame_table_bytes(self.total) // 4, dtype=torch.float32, device=self.device)
        torch.cuda.synchronize(self.device)
        ctx.normalize_device(self.d_kp.data_ptr(), self.d_frame_off.data_ptr(), self.d_wh.data_ptr(), self.n_frames, self.total,
                             self.d_pts.data_ptr())
        ctx.synchronize()
        return self


class DescriptorTable:
    """Descriptors of all frames of a sequence, resident on the GPU beside a FrameTable (descriptor i of a frame belongs to
    keypoint i). kind = GMS_DESC_HAMMING256: uint8 [n, 32] rows (ORB); GMS_DESC_L2_F32X128: float32 [n, 128] rows (SIFT), for
    which the per-frame tables of the matcher are prepared once here (gms_bf_prepare_device)."""

    def __init__(self, ctx, frames, descriptors_per_frame, kind):
        self.ctx, self.kind, self.frames = ctx, int(kind), frames
        dt, width = desc_layout(self.kind)
        rows = [np.ascontiguousarray(d, dtype=dt).reshape(-1, width) for d in descriptors_per_frame]
        assert [len(r) for r in rows] == list(np.diff(frames.frame_off_host)), "one descriptor per keypoint"
        self.host = np.concatenate(rows) if frames.total else np.zeros((0, width), dtype=dt)
        self.d_desc = torch.from_numpy(self.host.view(np.uint8).reshape(-1)).to(frames.device) if frames.total else \
            torch.zeros(16, dtype=torch.uint8, device=frames.device)
        nbytes = ctx.bf_prepared_bytes(self.kind, frames.total, frames.n_frames)
        self.d_prep = torch.zeros(max(nbytes, 16), dtype=torch.uint8, device=frames.device)
        torch.cuda.synchronize(frames.device)
        ctx.bf_prepare_device(self.kind, self.d_desc.data_ptr(), frames.d_frame_off.data_ptr(), frames.n_frames, frames.total,
                              self.d_prep.data_ptr())
        ctx.synchronize()

    @classmethod
    def from_device(cls, frames, d_rows, kind):
        """The table of rows that are on the device already: d_rows a tensor of frames.total rows (or more: the head is used), row i
        belonging to keypoint i of `frames`. Nothing is read back; `host` is None."""
        self = cls.__new__(cls)
        self.ctx, self.kind, self.frames, self.host = frames.ctx, int(kind), frames, None
        dt, width = desc_layout(self.kind)
        self.d_desc = d_rows.contiguous().view(torch.uint8).reshape(-1)
        if self.d_desc.numel() < frames.total * width * np.dtype(dt).itemsize:
            raise ValueError("one descriptor per keypoint")
        if self.d_desc.numel() == 0:
            self.d_desc = torch.zeros(16, dtype=torch.uint8, device=frames.device)
        nbytes = self.ctx.bf_prepared_bytes(self.kind, frames.total, frames.n_frames)
        self.d_prep = torch.zeros(max(nbytes, 16), dtype=torch.uint8, device=frames.device)
        torch.cuda.synchronize(frames.device)
        self.ctx.bf_prepare_device(self.kind, self.d_desc.data_ptr(), frames.d_frame_off.data_ptr(), frames.n_frames, frames.total,
                                   self.d_prep.data_ptr())
        self.ctx.synchronize()
        return self

    def match_device(self, d_pairs, n_pairs, max_query, d_matches, use_prepared=True):
        """gms_bfmatch_device: one match per query row of every pair, written at the pair's match_off (stream-ordered).
        use_prepared=False (Hamming only): the vector-ALU kernel on the raw rows instead of the matrix-core one."""
        f = self.frames
        self.ctx.bfmatch_device(self.kind, self.d_desc.data_ptr(), self.d_prep.data_ptr() if use_prepared else None, f.total,
                                f.d_frame_off.data_ptr(), f.n_frames, d_pairs, n_pairs, max_query, d_matches)


class BfSelect:
    """Device buffers of one gms_bf_select_device batch over a DescriptorTable: the pair table, workspace, output and result
    records, sized once, so that run() can be replayed (or captured into a graph) on the same pairs."""

    def __init__(self, ctx, descs, recs, cross_check=True, distance_coef=4.0, max_size=500, use_prepared=True):
        f = descs.frames
        self.ctx, self.descs, self.recs = ctx, descs, np.ascontiguousarray(recs, dtype=PAIR_DTYPE)
        self.cross_check, self.distance_coef, self.max_size, self.use_prepared = bool(cross_check), float(distance_coef), int(max_size), use_prepared
        sizes = np.diff(f.frame_off_host)
        a, b = self.recs["frame_a"], self.recs["frame_b"]
        ok = (a >= 0) & (a < f.n_frames) & (b >= 0) & (b < f.n_frames)   # a pair with one bad index sizes nothing
        na, nb = np.where(ok, frame_counts(sizes, a), 0), np.where(ok, frame_counts(sizes, b), 0)
        self.max_rows = int(max(na.max(initial=0), nb.max(initial=0)))
        self.total_back = int((nb if self.cross_check else na).sum())
        n = len(self.recs)
        dev = f.device
        self.ws_bytes = ctx.bf_select_workspace_bytes(n, self.max_rows, self.total_back)
        self.d_ws = torch.zeros(max(self.ws_bytes, 256), dtype=torch.uint8, device=dev)
        self.d_pairs = _to_dev(self.recs, dev) if n else torch.zeros(24, dtype=torch.uint8, device=dev)
        total = int((self.recs["match_off"] + np.maximum(self.recs["m"], 0)).max()) if n else 0
        self.out_len = total
        self.d_out = torch.zeros(max(total, 1) * 16, dtype=torch.uint8, device=dev)
        self.d_res = torch.zeros(max(n, 1) * 32, dtype=torch.uint8, device=dev)
        self.d_pres = torch.zeros(max(n, 1) * 16, dtype=torch.uint8, device=dev)
        torch.cuda.synchronize(dev)

    def run(self):
        f, d = self.descs.frames, self.descs
        self.ctx.bf_select_device(d.kind, d.d_desc.data_ptr(), d.d_prep.data_ptr() if self.use_prepared else None, f.total,
                                  f.d_frame_off.data_ptr(), f.n_frames, self.d_pairs.data_ptr(), len(self.recs), self.max_rows,
                                  self.cross_check, self.distance_coef, self.max_size, self.d_ws.data_ptr(), self.ws_bytes,
                                  self.d_out.data_ptr(), self.d_res.data_ptr(), self.d_pres.data_ptr())

    def results(self):
        """(output DMATCH_DTYPE array laid out by match_off, BF_RESULT_DTYPE records, RESULT_DTYPE records) on the host."""
        n = len(self.recs)
        out = self.d_out.cpu().numpy().view(DMATCH_DTYPE)[: self.out_len].copy()
        return out, self.d_res.cpu().numpy().view(BF_RESULT_DTYPE)[:n].copy(), self.d_pres.cpu().numpy().view(RESULT_DTYPE)[:n].copy()


def bf_select_table(descs, frame_pairs, capacity=None, max_size=500):
    """PAIR_DTYPE records for (frame_a, frame_b) pairs; m: output room per pair (int or one per pair; default min(max_size, n_a),
    which K never exceeds), match_off: the running sum."""
    fp = np.asarray(frame_pairs, dtype=np.int64).reshape(-1, 2)
    if capacity is None:
        capacity = np.minimum(frame_counts(np.diff(descs.frames.frame_off_host), fp[:, 0]), max(int(max_size), 0))
    return pair_table(fp, capacity)


def bf_select_pairs(ctx, descs, frame_pairs, cross_check=True, distance_coef=4.0, max_size=500, capacity=None, use_prepared=True):
    """The reference's bruteForceMatch (FeatureMatchUtil.cpp:20-31) for every (frame_a, frame_b) pair of a DescriptorTable: (list of
    DMATCH_DTYPE survivor arrays, BF_RESULT_DTYPE records). Pairs that come back with GMS_ERR_CAPACITY are run once more with the
    count they reported."""
    def run(recs):
        job = BfSelect(ctx, descs, recs, cross_check, distance_coef, max_size, use_prepared)
        job.run()
        ctx.synchronize()
        return job.results()[:2]

    return run_with_retry(bf_select_table(descs, frame_pairs, capacity, max_size), run)


def _image_stack(ctx, images, device):
    dev = _device(ctx, device)
    imgs = images if torch.is_tensor(images) else torch.from_numpy(np.ascontiguousarray(images, dtype=np.uint8))
    if imgs.dim() == 2:
        imgs = imgs[None]
    return dev, imgs.to(dev).contiguous()


def _detected(d_kp, d_desc, d_counts, n, max_keypoints):
    """(keypoints_per_image, rows_per_image) on the host from a detector's [n, max_keypoints] record and row buffers and its counts."""
    counts = d_counts.cpu().numpy()
    kp = d_kp.cpu().numpy()[: n * max_keypoints * 28].view(KEYPOINT_DTYPE).reshape(n, max_keypoints)
    desc = d_desc.cpu().numpy()[: n * max_keypoints * 32].reshape(n, max_keypoints, 32)
    return [kp[i, : counts[i]].copy() for i in range(n)], [desc[i, : counts[i]].copy() for i in range(n)]


def detect_images(ctx, images, threshold=20, max_keypoints=10000, device=None):
    """gms_detect_batch_device on a stack of equally sized 8-bit grey images [n, H, W] (host array or device tensor): returns
    (keypoints_per_image, rows_per_image) as host arrays -- KEYPOINT_DTYPE records in raster order and uint8 [n_i, 32] rows."""
    dev, imgs = _image_stack(ctx, images, device)
    n, h, w = imgs.shape
    nb = ctx.detect_workspace_bytes(w, h, n, max_keypoints)
    if nb == 0:
        raise ValueError("bad image size")
    d_ws = torch.zeros(nb, dtype=torch.uint8, device=dev)
    d_kp = torch.zeros(max(n * max_keypoints, 1) * 28, dtype=torch.uint8, device=dev)
    d_desc = torch.zeros(max(n * max_keypoints, 1) * 32, dtype=torch.uint8, device=dev)
    d_counts = torch.zeros(n, dtype=torch.int32, device=dev)
    torch.cuda.synchronize(dev)
    ctx.detect_batch_device(imgs.data_ptr(), n, w, h, threshold, max_keypoints, d_ws.data_ptr(), nb, d_kp.data_ptr(), d_desc.data_ptr(),
                            d_counts.data_ptr())
    ctx.synchronize()
    return _detected(d_kp, d_desc, d_counts, n, max_keypoints)


DESCRIPTORS = ("brief", "grad", "both")
DETECTORS = ("fast", "dog")
# (detector, refine, 128-float rows) -> the stem of the Context's <stem>_workspace_bytes and <stem>_batch_device; every entry point
# but detect_pyramid_batch_device ends with d_rows128 (None to the DoG calls: no such rows)
_PYRAMID_CALLS = {("fast", False, False): "detect_pyramid", ("fast", False, True): "detect_pyramid_grad",
                  ("dog", False, False): "detect_dog", ("dog", False, True): "detect_dog",
                  ("dog", True, False): "detect_dog_refined", ("dog", True, True): "detect_dog_refined"}


class DetectPyramid:
    """Device buffers of one gms_detect_pyramid_batch_device batch (n images of w x h), sized once, so that run() can be repeated or
    captured into a graph: workspace, keypoints, rows, counts and per-level counts. descriptor: "brief" (the 32-byte rows), "grad" or
    "both" (gms_detect_pyramid_grad_batch_device: the 128-float gradient rows as well, in d_rows128). detector: "fast" (the FAST-9
    corners of those two calls; `contrast` is not read) or "dog" (gms_detect_dog_batch_device: difference-of-Gaussians blobs with
    |D| > contrast, in 1/256 grey level; `threshold` is not read). Everything behind the candidates is the same for both.
    refine=True (detector "dog" only; gms_detect_dog_refined_batch_device): x, y and size of every record are refined to 1/16 pixel
    and 1/16 layer; nothing else of the output changes."""

    def __init__(self, ctx, n, w, h, threshold=20, max_keypoints=10000, n_levels=8, device=None, descriptor="brief", detector="fast",
                 contrast=128, refine=False):
        if descriptor not in DESCRIPTORS:
            raise ValueError(f"descriptor must be one of {DESCRIPTORS}")
        if detector not in DETECTORS:
            raise ValueError(f"detector must be one of {DETECTORS}")
        if refine and detector != "dog":
            raise ValueError('refine=True needs detector="dog"')
        self.refine = bool(refine)
        self.ctx, self.n, self.w, self.h, self.descriptor, self.detector = ctx, int(n), int(w), int(h), descriptor, detector
        self.threshold, self.max_keypoints, self.n_levels, self.contrast = int(threshold), int(max_keypoints), int(n_levels), int(contrast)
        dev = _device(ctx, device)
        stem = _PYRAMID_CALLS[detector, self.refine, descriptor != "brief"]
        self._call, self._takes_rows128 = getattr(ctx, stem + "_batch_device"), stem != "detect_pyramid"
        self.ws_bytes = getattr(ctx, stem + "_workspace_bytes")(w, h, n, max_keypoints, n_levels)
        if self.ws_bytes == 0:
            raise ValueError("bad image size, keypoint count or number of levels")
        self.d_ws = torch.zeros(self.ws_bytes, dtype=torch.uint8, device=dev)
        self.d_kp = torch.zeros(max(self.n * self.max_keypoints, 1) * 28, dtype=torch.uint8, device=dev)
        self.d_desc = torch.zeros(max(self.n * self.max_keypoints, 1) * 32, dtype=torch.uint8, device=dev)
        self.d_counts = torch.zeros(self.n, dtype=torch.int32, device=dev)
        self.d_level_counts = torch.zeros(self.n * self.n_levels, dtype=torch.int32, device=dev)
        self.d_rows128 = None if descriptor == "brief" else torch.zeros(max(self.n * self.max_keypoints, 1) * 128, dtype=torch.float32, device=dev)
        torch.cuda.synchronize(dev)

    def run(self, d_images):
        """Stream-ordered on the context's stream; d_images: uint8 device tensor [n, h, w], contiguous."""
        strength = self.contrast if self.detector == "dog" else self.threshold
        args = (d_images.data_ptr(), self.n, self.w, self.h, strength, self.max_keypoints, self.n_levels, self.d_ws.data_ptr(), self.ws_bytes,
                self.d_kp.data_ptr(), self.d_desc.data_ptr(), self.d_counts.data_ptr(), self.d_level_counts.data_ptr())
        if self._takes_rows128:
            args += (None if self.d_rows128 is None else self.d_rows128.data_ptr(),)
        self._call(*args)

    def results(self):
        """On the host: (keypoints_per_image, rows_per_image, level_counts [n, n_levels]); rows_per_image are the uint8 [n_i, 32] rows for
        "brief" and the float32 [n_i, 128] rows for "grad"; "both" gives (keypoints, rows32, rows128, level_counts)."""
        kps, rows32 = _detected(self.d_kp, self.d_desc, self.d_counts, self.n, self.max_keypoints)
        level_counts = self.d_level_counts.cpu().numpy().reshape(self.n, self.n_levels).copy()
        if self.d_rows128 is None:
            return kps, rows32, level_counts
        grad = self.d_rows128.cpu().numpy()[: self.n * self.max_keypoints * 128].reshape(self.n, self.max_keypoints, 128)
        rows128 = [grad[i, : len(kps[i])].copy() for i in range(self.n)]
        return (kps, rows128, level_counts) if self.descriptor == "grad" else (kps, rows32, rows128, level_counts)


def detect_images_pyramid(ctx, images, threshold=20, max_keypoints=10000, n_levels=8, device=None, descriptor="brief", detector="fast",
                          contrast=128, refine=False):
    """gms_detect_pyramid_batch_device on a stack of equally sized 8-bit grey images [n, H, W]: the detector of detect_images on every
    level of an image pyramid (ratio about 1.2). Returns (keypoints_per_image, rows_per_image, level_counts [n, n_levels]) as host
    arrays: KEYPOINT_DTYPE records in level-0 pixel coordinates with size and octave, level 0 first, raster order inside a level.
    descriptor="grad": rows_per_image are the float32 [n_i, 128] gradient rows (for GMS_DESC_L2_F32X128); "both": (keypoints, 32-byte
    rows, 128-float rows, level_counts). detector="dog": the keypoints are difference-of-Gaussians blobs (gms_detect_dog_batch_device,
    `contrast` in 1/256 grey level in the place of `threshold`); the outputs have the same form. refine=True (with "dog"):
    gms_detect_dog_refined_batch_device, the same records with x, y and size refined."""
    dev, imgs = _image_stack(ctx, images, device)
    n, h, w = imgs.shape
    run = DetectPyramid(ctx, n, w, h, threshold, max_keypoints, n_levels, dev, descriptor, detector, contrast, refine)
    run.run(imgs)
    ctx.synchronize()
    return run.results()


def dog_candidates(ctx, images, contrast=128, device=None):
    """gms_dog_candidates_device on a stack of equally sized 8-bit grey images [n, H, W]: the DoG detector's candidate planes on the
    images themselves (one level, before any selection) as a host array uint8 [n, H, W] -- the score 1..255 at a candidate, else 0."""
    dev, imgs = _image_stack(ctx, images, device)
    n, h, w = imgs.shape
    d_cand = torch.zeros((n, h, w), dtype=torch.uint8, device=dev)
    torch.cuda.synchronize(dev)
    ctx.dog_candidates_device(imgs.data_ptr(), n, w, h, contrast, d_cand.data_ptr())
    ctx.synchronize()
    return d_cand.cpu().numpy()


def dog_offsets(ctx, images, contrast=128, device=None):
    """gms_dog_offsets_device on a stack of equally sized 8-bit grey images [n, H, W]: the refinement's code planes on the images
    themselves (one level) as a host array uint16 [n, H, W] -- 1 + (ox + 8) + 17 (oy + 8) + 289 (os + 8) at a candidate of
    dog_candidates, the offsets in 1/16 pixel and 1/16 layer, else 0."""
    dev, imgs = _image_stack(ctx, images, device)
    n, h, w = imgs.shape
    d_codes = torch.zeros((n, h, w), dtype=torch.int16, device=dev)
    torch.cuda.synchronize(dev)
    ctx.dog_offsets_device(imgs.data_ptr(), n, w, h, contrast, d_codes.data_ptr())
    ctx.synchronize()
    return d_codes.cpu().numpy().view(np.uint16)


def bgr_to_gray(ctx, d_bgr):
    """gms_bgr_to_gray_device on a uint8 device tensor [n, H, W, 3] (B, G, R; contiguous) -> the grey planes, a device tensor
    [n, H, W]: (299 R + 587 G + 114 B + 500) // 1000. Stream-ordered on the context's stream."""
    n, h, w, _ = d_bgr.shape
    d_gray = torch.zeros((n, h, w), dtype=torch.uint8, device=d_bgr.device)
    torch.cuda.synchronize(d_bgr.device)
    ctx.bgr_to_gray_device(d_bgr.data_ptr(), n, w, h, d_gray.data_ptr())
    return d_gray


def pack_detector(run):
    """gms_detect_pack_device on a DetectPyramid that has run: (d_kp, d_rows32, d_rows128, d_frame_off) -- the images' records and rows
    back to back in tensors with room for n * max_keypoints of them, and the int64 [n + 1] offsets; d_rows128 is None for "brief".
    Stream-ordered on the context's stream; nothing is read back."""
    dev, slots = run.d_kp.device, max(run.n * run.max_keypoints, 1)
    d_kp = torch.zeros(slots * 28, dtype=torch.uint8, device=dev)
    d_rows32 = torch.zeros(slots * 32, dtype=torch.uint8, device=dev)
    d_rows128 = None if run.d_rows128 is None else torch.zeros(slots * 128, dtype=torch.float32, device=dev)
    d_frame_off = torch.zeros(run.n + 1, dtype=torch.int64, device=dev)
    torch.cuda.synchronize(dev)
    run.ctx.detect_pack_device(run.d_kp.data_ptr(), run.d_desc.data_ptr(), None if d_rows128 is None else run.d_rows128.data_ptr(),
                               run.d_counts.data_ptr(), run.n, run.max_keypoints, d_kp.data_ptr(), d_rows32.data_ptr(),
                               None if d_rows128 is None else d_rows128.data_ptr(), d_frame_off.data_ptr())
    return d_kp, d_rows32, d_rows128, d_frame_off


def tables_from_detector(run, sizes=None, kind=None):
    """(FrameTable, DescriptorTable) of a DetectPyramid that has run, without its keypoints or rows passing through the host: the
    blocks are packed on the device (gms_detect_pack_device), the n + 1 offsets are read back, the tables are built on the packed
    tensors. sizes: one (width, height) per image (default: the detector's). kind: GMS_DESC_HAMMING256 (the 32-byte rows) or
    GMS_DESC_L2_F32X128 (the gradient rows; the detector must have made them); default: L2 where there are gradient rows."""
    if kind is None:
        kind = GMS_DESC_HAMMING256 if run.d_rows128 is None else GMS_DESC_L2_F32X128
    desc_layout(kind)
    if int(kind) == GMS_DESC_L2_F32X128 and run.d_rows128 is None:
        raise ValueError('GMS_DESC_L2_F32X128 needs a detector with descriptor="grad" or "both"')
    d_kp, d_rows32, d_rows128, d_frame_off = pack_detector(run)
    frames = FrameTable.from_device(run.ctx, d_kp, d_frame_off, [(run.w, run.h)] * run.n if sizes is None else sizes)
    return frames, DescriptorTable.from_device(frames, d_rows32 if int(kind) == GMS_DESC_HAMMING256 else d_rows128, kind)


def build_pyramid(ctx, images, n_levels=8, device=None):
    """gms_pyramid_build_device: the level images of a stack [n, H, W] -> a list over the levels of host arrays [n, h_l, w_l] (level 0:
    the input itself)."""
    dev, imgs = _image_stack(ctx, images, device)
    n, h, w = imgs.shape
    sizes = ctx.pyramid_level_sizes(w, h, n_levels)
    nb = n * sum(wl * hl for wl, hl in sizes[1:])
    d_levels = torch.zeros(max(nb, 1), dtype=torch.uint8, device=dev)
    torch.cuda.synchronize(dev)
    ctx.pyramid_build_device(imgs.data_ptr(), n, w, h, n_levels, d_levels.data_ptr(), nb)
    ctx.synchronize()
    flat, out, off = d_levels.cpu().numpy(), [imgs.cpu().numpy()], 0
    for wl, hl in sizes[1:]:
        out.append(flat[off:off + n * wl * hl].reshape(n, hl, wl).copy())
        off += n * wl * hl
    return out


def describe_image(ctx, image, keypoints, device=None, descriptor="brief", fill=0):
    """gms_describe_device: directions and 32-byte rows at the given integer keypoints of one image -> (status, keypoints, rows).
    descriptor="grad": gms_describe_grad_device, float32 [n, 128] rows. fill: what the rows hold before the call (a refused keypoint's
    row keeps it)."""
    if descriptor not in ("brief", "grad"):
        raise ValueError('descriptor must be "brief" or "grad"')
    dev = _device(ctx, device)
    img = torch.from_numpy(np.ascontiguousarray(image, dtype=np.uint8)).to(dev)
    h, w = img.shape
    kp = np.ascontiguousarray(keypoints, dtype=KEYPOINT_DTYPE)
    nb = ctx.detect_workspace_bytes(w, h, 1, 0)
    if nb == 0:
        raise ValueError("bad image size")
    d_ws = torch.zeros(nb, dtype=torch.uint8, device=dev)
    d_kp = _to_dev(kp, dev) if len(kp) else torch.zeros(28, dtype=torch.uint8, device=dev)
    grad = descriptor == "grad"
    width = 128 if grad else 32
    d_desc = torch.full((max(len(kp), 1) * width,), fill, dtype=torch.float32 if grad else torch.uint8, device=dev)
    d_status = torch.zeros(1, dtype=torch.int32, device=dev)
    torch.cuda.synchronize(dev)
    call = ctx.describe_grad_device if grad else ctx.describe_device
    call(img.data_ptr(), w, h, d_kp.data_ptr(), len(kp), d_ws.data_ptr(), nb, d_desc.data_ptr(), d_status.data_ptr())
    ctx.synchronize()
    out_kp = d_kp.cpu().numpy()[: len(kp) * 28].view(KEYPOINT_DTYPE).copy() if len(kp) else kp
    return int(d_status.item()), out_kp, d_desc.cpu().numpy()[: len(kp) * width].reshape(-1, width)


def match_pairs(ctx, descs, pairs, use_prepared=True):
    """Brute-force matches of `pairs` (PAIR_DTYPE; m = keypoints of frame_a) as a host DMATCH_DTYPE array laid out by match_off."""
    dev = descs.frames.device
    pairs = np.ascontiguousarray(pairs, dtype=PAIR_DTYPE)
    total = int((pairs["match_off"] + pairs["m"]).max()) if len(pairs) else 0
    d_pairs = _to_dev(pairs, dev)
    d_matches = torch.zeros(max(total, 1) * 16, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize(dev)
    descs.match_device(d_pairs.data_ptr(), len(pairs), int(pairs["m"].max()) if len(pairs) else 0, d_matches.data_ptr(), use_prepared)
    ctx.synchronize()
    return d_matches.cpu().numpy().view(DMATCH_DTYPE)[:total]


def filter_pairs(ctx, frames, pairs, matches, withRotation=False, withScale=False, thresholdFactor=6.0,
                 want_mask=True):
    """Run the filter over `pairs` (PAIR_DTYPE array) whose matches live in `matches` (DMATCH_DTYPE array,
    pair i at [match_off, match_off+m)). Returns (out, results, mask) as host arrays."""
    dev = frames.device
    pairs = np.ascontiguousarray(pairs, dtype=PAIR_DTYPE)
    matches = np.ascontiguousarray(matches, dtype=DMATCH_DTYPE)
    n_pairs = len(pairs)
    max_m = int(pairs["m"].max()) if n_pairs else 0
    total_m = len(matches)
    d_pairs = _to_dev(pairs, dev)
    d_matches = _to_dev(matches, dev) if total_m else torch.zeros(16, dtype=torch.uint8, device=dev)
    d_out = torch.zeros(max(total_m, 1) * 16, dtype=torch.uint8, device=dev)
    d_res = torch.zeros(max(n_pairs, 1) * 16, dtype=torch.uint8, device=dev)
    d_mask = torch.zeros(max(total_m, 1), dtype=torch.uint8, device=dev) if want_mask else None
    torch.cuda.synchronize(dev)
    ctx.filter_device(frames.d_pts.data_ptr(), frames.d_frame_off.data_ptr(), frames.n_frames,
                      d_pairs.data_ptr(), n_pairs, max_m, d_matches.data_ptr(), d_out.data_ptr(),
                      d_res.data_ptr(), d_mask.data_ptr() if want_mask else None,
                      withRotation, withScale, thresholdFactor)
    ctx.synchronize()
    out = d_out.cpu().numpy().view(DMATCH_DTYPE)[:total_m]
    res = d_res.cpu().numpy().view(RESULT_DTYPE)[:n_pairs]
    mask = d_mask.cpu().numpy()[:total_m] if want_mask else None
    return out, res, mask


# ---- LOGOS on resident frames (gms_logos_*) --------------------------------------------------------------------------
class LogosTable:
    """The per-frame LOGOS table of a sequence (gms_logos_prepare_device): points, five nearest neighbours and word buckets of every
    frame, worked out once for all the pairs the frames are matched in.

    keypoints_per_frame: a list of KEYPOINT_DTYPE arrays, or a FrameTable whose resident keypoints are used. words_per_frame: one word
    per keypoint in [0, n_words) -- a list of per-frame int arrays, or an int32 device tensor of all keypoints back to back (as
    gms_logos_words_device leaves it). A frame with a word out of range, or with a keypoint outside the domain (pt.x, pt.y and angle
    finite, |angle| <= 3600 degrees; size is not restricted), is marked: its pairs come back with GMS_ERR_DOMAIN."""

    def __init__(self, ctx, keypoints_per_frame, words_per_frame, n_words, device="cuda:0"):
        self.ctx, self.n_words = ctx, int(n_words)
        if isinstance(keypoints_per_frame, FrameTable):
            ft = keypoints_per_frame
            self.device, self.n_frames, self.frame_off_host, self.total = ft.device, ft.n_frames, ft.frame_off_host, ft.total
            self.d_kp, self.d_frame_off = ft.d_kp, ft.d_frame_off
        else:
            self.device = torch.device(device)
            self.n_frames = len(keypoints_per_frame)
            kp_all, self.frame_off_host = concat_frames(keypoints_per_frame)
            self.total = int(self.frame_off_host[-1])
            self.d_kp = _to_dev(kp_all, self.device) if self.total else torch.zeros(28, dtype=torch.uint8, device=self.device)
            self.d_frame_off = torch.from_numpy(self.frame_off_host).to(self.device)
        self.counts = np.diff(self.frame_off_host)
        if torch.is_tensor(words_per_frame):
            self.d_words = words_per_frame.to(self.device, torch.int32).contiguous()
        else:
            w = (np.concatenate([np.asarray(x, dtype=np.int64).reshape(-1) for x in words_per_frame]) if len(words_per_frame)
                 else np.zeros(0, np.int64))
            if len(w) != self.total:
                raise ValueError("one word per keypoint")
            w = np.clip(w, -1, 2**31 - 1).astype(np.int32)   # (out of range stays out of range)
            self.d_words = torch.from_numpy(w).to(self.device) if self.total else torch.zeros(1, dtype=torch.int32, device=self.device)
        if self.d_words.numel() < self.total:
            raise ValueError("one word per keypoint")
        self.max_kp = int(self.counts.max()) if self.n_frames else 0
        self.d_table = torch.zeros(max(ctx.logos_table_bytes(self.total, self.n_frames, self.n_words), 16), dtype=torch.uint8,
                                   device=self.device)
        ws = ctx.logos_workspace_bytes(self.max_kp, 0, 0)
        d_ws = torch.empty(max(ws, 16), dtype=torch.uint8, device=self.device)
        torch.cuda.synchronize(self.device)
        ctx.logos_prepare_device(self.d_kp.data_ptr(), self.d_frame_off.data_ptr(), self.n_frames, self.total, self.d_words.data_ptr(),
                                 self.n_words, d_ws.data_ptr(), ws, self.d_table.data_ptr())
        ctx.synchronize()

    def filter_device(self, d_pairs, n_pairs, d_ws, ws_bytes, d_out, d_logos_results, d_pair_results=None):
        """gms_logos_filter_device on this table (stream-ordered; capturable)."""
        self.ctx.logos_filter_device(self.d_table.data_ptr(), d_pairs, n_pairs, d_ws, ws_bytes, d_out, d_logos_results, d_pair_results)


def logos_pair_table(table, frame_pairs, capacity=None):
    """PAIR_DTYPE records for (frame_a, frame_b) pairs: m = the output capacity (default max(n_a, n_b) per pair -- survivors rarely
    outnumber the larger frame), match_off back to back."""
    fp = np.asarray(frame_pairs, dtype=np.int64).reshape(-1, 2)
    if capacity is None:
        capacity = np.maximum(frame_counts(table.counts, fp[:, 0]), frame_counts(table.counts, fp[:, 1]))
    return pair_table(fp, capacity)


class LogosFilter:
    """Device buffers of one gms_logos_filter_device batch over a LogosTable: the pair table, workspace, output and both kinds of result
    records, sized once, so that run() can be replayed on the same pairs. A frame index out of range is the library's to report
    (GMS_ERR_BAD_ARG for that pair alone): it counts as an empty frame here."""

    def __init__(self, ctx, table, pairs):
        self.ctx, self.table, self.pairs = ctx, table, np.ascontiguousarray(pairs, dtype=PAIR_DTYPE)
        n, dev = len(self.pairs), table.device
        self.out_len = int((self.pairs["match_off"] + np.maximum(self.pairs["m"], 0)).max()) if n else 0
        max_q = int(frame_counts(table.counts, self.pairs["frame_a"]).max()) if n else 0
        self.ws_bytes = ctx.logos_workspace_bytes(0, n, max_q)
        self.d_pairs = _to_dev(self.pairs, dev) if n else torch.zeros(24, dtype=torch.uint8, device=dev)
        self.d_ws = torch.empty(max(self.ws_bytes, 16), dtype=torch.uint8, device=dev)
        self.d_out = torch.zeros(max(self.out_len, 1) * 16, dtype=torch.uint8, device=dev)
        self.d_lres = torch.zeros(max(n, 1) * LOGOS_RESULT_DTYPE.itemsize, dtype=torch.uint8, device=dev)
        self.d_pres = torch.zeros(max(n, 1) * RESULT_DTYPE.itemsize, dtype=torch.uint8, device=dev)
        torch.cuda.synchronize(dev)

    def run(self):
        self.table.filter_device(self.d_pairs.data_ptr(), len(self.pairs), self.d_ws.data_ptr(), self.ws_bytes, self.d_out.data_ptr(),
                                 self.d_lres.data_ptr(), self.d_pres.data_ptr())

    def logos_results(self):
        return self.d_lres.cpu().numpy().view(LOGOS_RESULT_DTYPE)[: len(self.pairs)].copy()

    def results(self):
        """(output DMATCH_DTYPE array laid out by match_off, LOGOS_RESULT_DTYPE records, RESULT_DTYPE records) on the host."""
        return (self.d_out.cpu().numpy().view(DMATCH_DTYPE)[: self.out_len], self.logos_results(),
                self.d_pres.cpu().numpy().view(RESULT_DTYPE)[: len(self.pairs)].copy())


def logos_filter(ctx, table, pairs):
    """One gms_logos_filter_device run over PAIR_DTYPE `pairs` -> (out, logos_results, pair_results) as host arrays (out laid out by
    match_off; pairs with GMS_ERR_CAPACITY wrote nothing)."""
    if len(pairs) == 0:
        return np.zeros(0, DMATCH_DTYPE), np.zeros(0, LOGOS_RESULT_DTYPE), np.zeros(0, RESULT_DTYPE)
    job = LogosFilter(ctx, table, pairs)
    job.run()
    ctx.synchronize()
    return job.results()


def logos_pairs(ctx, table, pairs, capacity=None):
    """The survivors of every (frame_a, frame_b) pair of `pairs` on a LogosTable: (list of DMATCH_DTYPE arrays, LOGOS_RESULT_DTYPE
    records). capacity: output room per pair (int or one per pair; default max(n_a, n_b)). Pairs that come back with
    GMS_ERR_CAPACITY are run once more with the count they reported, as matchLOGOS does for one pair."""
    return run_with_retry(logos_pair_table(table, pairs, capacity), lambda recs: logos_filter(ctx, table, recs)[:2])


def _words_device(ctx, kind, rows, dic, dev):
    """gms_logos_words_device on host rows and a host dictionary -> (int32 device tensor of one word per row, the device inputs).
    Stream-ordered on the context's stream and not waited for: the caller holds on to the inputs until it has synchronised."""
    d_desc = torch.from_numpy(rows.view(np.uint8).reshape(-1)).to(dev)
    d_dict = torch.from_numpy(dic.view(np.uint8).reshape(-1).copy()).to(dev)
    d_words = torch.zeros(len(rows), dtype=torch.int32, device=dev)
    torch.cuda.synchronize(dev)
    ctx.logos_words_device(kind, d_desc.data_ptr(), len(rows), d_dict.data_ptr(), len(dic), d_words.data_ptr())
    return d_words, (d_desc, d_dict)


def logos_words(ctx, descriptors_per_frame, dictionary, kind, device=None):
    """gms_logos_words_device: the exact nearest dictionary row (lowest index on ties) of every descriptor row -- in place of the
    reference's FLANN lookup (FeatureMatchUtil.cpp:86-131). descriptors_per_frame: a list of per-frame row arrays (or one array);
    kind GMS_DESC_L2_F32X128: float32 [n, 128] rows, GMS_DESC_HAMMING256: uint8 [n, 32]. Returns int32 words per frame."""
    dev = _device(ctx, device)
    kind = int(kind)
    dt, width = desc_layout(kind)
    single = not isinstance(descriptors_per_frame, (list, tuple))
    frames = [descriptors_per_frame] if single else list(descriptors_per_frame)
    rows = [np.ascontiguousarray(d, dtype=dt).reshape(-1, width) for d in frames]
    counts = [len(r) for r in rows]
    total = int(sum(counts))
    dic = np.ascontiguousarray(dictionary, dtype=dt).reshape(-1, width)
    words = np.zeros(0, np.int32)
    if total:
        d_words, held = _words_device(ctx, kind, np.concatenate(rows), dic, dev)
        ctx.synchronize()
        words = d_words.cpu().numpy()
    elif not 1 <= len(dic) <= 65535:
        raise ValueError("1 <= dictionary rows <= 65535")
    out = np.split(words, np.cumsum(counts)[:-1]) if counts else []
    return out[0] if single else out


class LogosDictionary:
    """Device buffers of gms_logos_dict_train_device for up to max_sets training sets of max_rows descriptor rows in all: the rows, the
    set offsets, workspace, dictionaries, records and labels, sized once, so that run() can be repeated -- or captured into a graph
    and replayed -- on new rows put into the same tensors (d_desc, d_set_off). The arguments that size the launches (n_sets, the row
    total, n_words, attempts, max_iters) are fixed here; the offsets are read on the device, so sets may change size between runs."""

    def __init__(self, ctx, kind, n_sets, total_rows, n_words=50, attempts=3, max_iters=100, seed=0, device=None):
        self.dtype, self.width = logos_dict_args(kind, n_words, attempts, max_iters)
        self.ctx, self.kind, self.n_sets, self.total_rows = ctx, int(kind), int(n_sets), int(total_rows)
        self.n_words, self.attempts, self.max_iters, self.seed = int(n_words), int(attempts), int(max_iters), int(seed)
        dev = _device(ctx, device)
        self.device = dev
        self.ws_bytes = ctx.logos_dict_workspace_bytes(self.kind, self.total_rows, self.n_sets, self.n_words, self.attempts, self.max_iters)
        if self.ws_bytes == 0:
            raise ValueError("LogosDictionary: arguments refused (include/gms.h)")
        row_bytes = self.width * np.dtype(self.dtype).itemsize
        self.d_desc = torch.zeros(max(self.total_rows, 1) * row_bytes, dtype=torch.uint8, device=dev)
        self.d_set_off = torch.zeros(self.n_sets + 1, dtype=torch.int64, device=dev)
        self.d_ws = torch.zeros(self.ws_bytes, dtype=torch.uint8, device=dev)
        self.d_dict = torch.zeros(max(self.n_sets, 1) * self.n_words * row_bytes, dtype=torch.uint8, device=dev)
        self.d_results = torch.zeros(max(self.n_sets, 1) * LOGOS_DICT_RESULT_DTYPE.itemsize, dtype=torch.uint8, device=dev)
        self.d_labels = torch.full((max(self.total_rows, 1),), -1, dtype=torch.int32, device=dev)
        torch.cuda.synchronize(dev)

    def load(self, descriptor_sets):
        """Copy the rows of `descriptor_sets` (a list of row arrays, n_sets of them, total_rows rows in all at most) and their offsets
        into the device tensors (on the current torch stream)."""
        rows = [np.ascontiguousarray(d, dtype=self.dtype).reshape(-1, self.width) for d in descriptor_sets]
        if len(rows) != self.n_sets or sum(len(r) for r in rows) > self.total_rows:
            raise ValueError("LogosDictionary.load: n_sets sets of at most total_rows rows in all")
        off = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int64)
        if off[-1]:
            flat = torch.from_numpy(np.concatenate(rows).view(np.uint8).reshape(-1))
            self.d_desc[: flat.numel()].copy_(flat)
        self.d_set_off.copy_(torch.from_numpy(off))
        self.d_labels.fill_(-1)
        return off

    def run(self, with_labels=True):
        """gms_logos_dict_train_device on the tensors as they are: stream-ordered on the context's stream, capturable."""
        self.ctx.logos_dict_train_device(self.kind, self.d_desc.data_ptr(), self.d_set_off.data_ptr(), self.n_sets, self.total_rows,
                                         self.n_words, self.attempts, self.max_iters, self.seed, self.d_ws.data_ptr(), self.ws_bytes,
                                         self.d_dict.data_ptr(), self.d_results.data_ptr(), self.d_labels.data_ptr() if with_labels else None)

    def results(self):
        """(dictionaries [n_sets, n_words, width], LOGOS_DICT_RESULT_DTYPE records, labels per row) as host arrays."""
        dic = self.d_dict.cpu().numpy().view(self.dtype).reshape(max(self.n_sets, 1), self.n_words, self.width)[: self.n_sets]
        rec = self.d_results.cpu().numpy().view(LOGOS_DICT_RESULT_DTYPE)[: self.n_sets]
        return dic.copy(), rec.copy(), self.d_labels.cpu().numpy()[: self.total_rows]


def logos_dictionary(ctx, descriptor_sets, kind, n_words=50, attempts=3, max_iters=100, seed=0, device=None):
    """One dictionary per training set, all sets in the same launches (gms_logos_dict_train_device). descriptor_sets: a
    list of row arrays (or one array: one set). Returns (dictionaries [n_sets, n_words, width], LOGOS_DICT_RESULT_DTYPE records,
    list of int32 labels per set); a set that fails its checks has status != 0 in its record, a zero dictionary and labels -1."""
    single = not isinstance(descriptor_sets, (list, tuple))
    sets = [descriptor_sets] if single else list(descriptor_sets)
    dt, width = logos_dict_args(kind, n_words, attempts, max_iters)
    total = sum(len(np.asarray(d).reshape(-1, width)) for d in sets)
    job = LogosDictionary(ctx, kind, len(sets), total, n_words, attempts, max_iters, seed, device)
    off = job.load(sets)
    torch.cuda.synchronize(job.device)
    job.run()
    ctx.synchronize()
    dic, rec, labels = job.results()
    return dic, rec, [labels[off[s]:off[s + 1]] for s in range(len(sets))]


class StereoBM:
    """Device buffers of gms_stereo_bm_device for n pairs of one size: workspace, int16 maps, costs and 8-bit maps, sized once, so that
    run() can be replayed (or captured into a graph) on new images in the same tensors."""
    NAME = "StereoBM"
    make_params = staticmethod(stereo_bm_params)

    def _workspace_bytes(self):
        return self.ctx.stereo_bm_workspace_bytes(self.width, self.height, self.n, self.params)

    def _device_call(self, *args):
        self.ctx.stereo_bm_device(*args)

    def __init__(self, ctx, n, width, height, params=None, device="cuda:0", with_cost=True):
        self.ctx, self.n, self.width, self.height = ctx, int(n), int(width), int(height)
        self.params = self.make_params(params)
        dev = torch.device(device)
        self.ws_bytes = self._workspace_bytes()
        if self.ws_bytes == 0 and self.n > 0:
            raise ValueError(f"{self.NAME}: parameters or image size rejected (include/gms.h)")
        self.d_ws = torch.zeros(max(self.ws_bytes, 256), dtype=torch.uint8, device=dev)
        self.d_disp = torch.zeros((max(self.n, 1), self.height, self.width), dtype=torch.int16, device=dev)
        self.d_cost = torch.zeros((max(self.n, 1), self.height, self.width), dtype=torch.int32, device=dev) if with_cost else None
        self.d_out8 = torch.zeros((max(self.n, 1), self.height, self.width), dtype=torch.uint8, device=dev)
        torch.cuda.synchronize(dev)

    def run(self, d_left, d_right, eight_bit=False):
        """d_left / d_right: uint8 device tensors [n, height, width] (contiguous). Stream-ordered on the context's stream."""
        for t in (d_left, d_right):
            if t.dtype != torch.uint8 or tuple(t.shape) != (self.n, self.height, self.width) or not t.is_contiguous():
                raise ValueError("left / right: contiguous uint8 device tensors [n, height, width]")
        self._device_call(self.params, d_left.data_ptr(), d_right.data_ptr(), self.n, self.width, self.height, self.width,
                          self.d_ws.data_ptr(), self.ws_bytes, self.d_disp.data_ptr(),
                          self.d_cost.data_ptr() if self.d_cost is not None else None)
        if eight_bit:
            self.ctx.stereo_bm_normalize_device(self.d_disp.data_ptr(), self.n, self.width, self.height, self.d_out8.data_ptr())


class StereoSGM(StereoBM):
    """The same buffers for gms_stereo_sgm_device (semi-global matching on StereoBM's costs): the workspace also holds
    the two cost volumes, 4 * num_disparities bytes per pixel of the computed region."""
    NAME = "StereoSGM"
    make_params = staticmethod(stereo_sgm_params)

    def _workspace_bytes(self):
        return self.ctx.stereo_sgm_workspace_bytes(self.width, self.height, self.n, self.params)

    def _device_call(self, *args):
        self.ctx.stereo_sgm_device(*args)


def _stereo_batch(cls, lefts, rights, params, ctx, return_cost, eight_bit):
    from .api import default_context
    ctx = ctx or default_context()
    on_dev = isinstance(lefts, torch.Tensor)
    if on_dev:
        dl, dr = lefts.contiguous(), rights.contiguous()
    else:
        l, r = np.ascontiguousarray(lefts, dtype=np.uint8), np.ascontiguousarray(rights, dtype=np.uint8)
        if l.ndim != 3 or r.shape != l.shape:
            raise ValueError("lefts / rights: uint8 [n, H, W] of one shape")
        dl, dr = torch.from_numpy(l).cuda(), torch.from_numpy(r).cuda()
    n, h, w = dl.shape
    run = cls(ctx, n, w, h, params, dl.device, with_cost=return_cost)
    run.run(dl, dr, eight_bit)
    ctx.synchronize()
    outs = [run.d_disp[:n]] + ([run.d_cost[:n]] if return_cost else []) + ([run.d_out8[:n]] if eight_bit else [])
    if not on_dev:
        outs = [o.cpu().numpy() for o in outs]
    return outs[0] if len(outs) == 1 else tuple(outs)


def stereo_bm_batch(lefts, rights, params=None, ctx=None, return_cost=False, eight_bit=False):
    """StereoBM::compute for n pairs in one gms_stereo_bm_device run. lefts / rights: uint8 [n, H, W] host arrays or device tensors.
    Returns the int16 maps [n, H, W] (numpy for host input, device tensors for device input), then the int32 costs with
    return_cost=True and the reference's 8-bit maps with eight_bit=True."""
    return _stereo_batch(StereoBM, lefts, rights, params, ctx, return_cost, eight_bit)


def stereo_sgm_batch(lefts, rights, params=None, ctx=None, return_cost=False, eight_bit=False):
    """Semi-global matching for n pairs in one gms_stereo_sgm_device run: arguments and results as stereo_bm_batch's; params may also
    hold p1, p2 and n_paths (types.stereo_sgm_params)."""
    return _stereo_batch(StereoSGM, lefts, rights, params, ctx, return_cost, eight_bit)


class Portrait:
    """Device buffers of gms_portrait_device for n images of one size: workspace, portrait images and (with detail) the dilated masks,
    the selections and the blurred images, sized once, so that run() can be replayed (or captured into a graph) on new images in the
    same tensors."""

    def __init__(self, ctx, n, width, height, params=None, device="cuda:0", detail=True):
        self.ctx, self.n, self.width, self.height = ctx, int(n), int(width), int(height)
        self.params = portrait_params(params)
        dev = torch.device(device)
        self.ws_bytes = ctx.portrait_workspace_bytes(width, height, n, self.params)
        if self.ws_bytes == 0:
            raise ValueError("Portrait: parameters, image size or batch size rejected (include/gms.h)")
        self.d_ws = torch.zeros(self.ws_bytes, dtype=torch.uint8, device=dev)
        self.d_out = torch.zeros((self.n, self.height, self.width, 3), dtype=torch.uint8, device=dev)
        self.d_mask = torch.zeros((self.n, self.height, self.width), dtype=torch.uint8, device=dev) if detail else None
        self.d_selected = torch.zeros((self.n, self.height, self.width), dtype=torch.uint8, device=dev) if detail else None
        self.d_blurred = torch.zeros((self.n, self.height, self.width, 3), dtype=torch.uint8, device=dev) if detail else None
        torch.cuda.synchronize(dev)

    def run(self, d_bgr, d_disparity):
        """d_bgr: uint8 device tensor [n, height, width, 3]; d_disparity: [n, height, width] (both contiguous). Stream-ordered on the
        context's stream."""
        for t, shape in ((d_bgr, (self.n, self.height, self.width, 3)), (d_disparity, (self.n, self.height, self.width))):
            if t.dtype != torch.uint8 or tuple(t.shape) != shape or not t.is_contiguous():
                raise ValueError("images [n, height, width, 3] and disparities [n, height, width]: contiguous uint8 device tensors")
        opt = [t.data_ptr() if t is not None else None for t in (self.d_mask, self.d_selected, self.d_blurred)]
        self.ctx.portrait_device(self.params, d_bgr.data_ptr(), d_disparity.data_ptr(), self.n, self.width, self.height, 3 * self.width,
                                 self.width, self.d_ws.data_ptr(), self.ws_bytes, self.d_out.data_ptr(), *opt)


def portrait_batch(images, disparities, params=None, ctx=None, detail=False):
    """Portrait mode for n images in one gms_portrait_device run. images: uint8 [n, H, W, 3] (BGR); disparities: uint8 [n, H, W], 255 =
    no value; host arrays or device tensors. Returns the portrait images [n, H, W, 3] (numpy for host input, device tensors for device
    input); with detail=True (out, mask, selected, blurred)."""
    from .api import default_context
    ctx = ctx or default_context()
    on_dev = isinstance(images, torch.Tensor)
    if on_dev:
        di, dd = images.contiguous(), disparities.contiguous()
    else:
        im, dp = np.ascontiguousarray(images, dtype=np.uint8), np.ascontiguousarray(disparities, dtype=np.uint8)
        if im.ndim != 4 or im.shape[3] != 3 or dp.shape != im.shape[:3]:
            raise ValueError("images: uint8 [n, H, W, 3]; disparities: uint8 [n, H, W]")
        di, dd = torch.from_numpy(im).cuda(), torch.from_numpy(dp).cuda()
    n, h, w = dd.shape
    run = Portrait(ctx, n, w, h, params, di.device, detail=detail)
    run.run(di, dd)
    ctx.synchronize()
    outs = [run.d_out] + ([run.d_mask, run.d_selected, run.d_blurred] if detail else [])
    if not on_dev:
        outs = [o.cpu().numpy() for o in outs]
    return outs[0] if len(outs) == 1 else tuple(outs)


class Warp:
    """Device buffers of gms_resize_device / gms_warp_affine_device for n images of one size and channel count (1: [n, H, W]; 3:
    [n, H, W, 3]): the destination d_dst and, for warpAffine, the forward matrices d_M [n_matrices, 6] (n_matrices 1: one for all
    images, or n), sized once, so that the calls can be repeated or captured into a graph. The kernel reads d_M when it runs: a
    captured graph follows set_matrices()."""

    def __init__(self, ctx, n, src_size, dst_size, channels=1, n_matrices=1, device=None):
        self.ctx, self.n, self.channels, self.n_matrices = ctx, int(n), int(channels), int(n_matrices)
        (self.sw, self.sh), (self.dw, self.dh) = (int(v) for v in src_size), (int(v) for v in dst_size)
        if self.channels not in (1, 3) or self.n < 1 or min(self.sw, self.sh, self.dw, self.dh) < 1 or self.n_matrices not in (1, self.n):
            raise ValueError("Warp: channels 1 or 3, n >= 1, positive sizes, n_matrices 1 or n")
        dev = _device(ctx, device)
        tail = () if self.channels == 1 else (3,)
        self.src_shape = (self.n, self.sh, self.sw) + tail
        self.d_dst = torch.zeros((self.n, self.dh, self.dw) + tail, dtype=torch.uint8, device=dev)
        self.d_M = torch.zeros((self.n_matrices, 6), dtype=torch.float64, device=dev)
        torch.cuda.synchronize(dev)

    def set_matrices(self, M):
        """Forward 2 x 3 matrices, [n_matrices, 6] or [n_matrices, 2, 3] on the host -> d_M (a copy on torch's current stream)."""
        m = np.ascontiguousarray(M, dtype=np.float64).reshape(self.n_matrices, 6)
        self.d_M.copy_(torch.from_numpy(m))

    def _src(self, d_src):
        if d_src.dtype != torch.uint8 or tuple(d_src.shape) != self.src_shape or not d_src.is_contiguous():
            raise ValueError(f"images: a contiguous uint8 device tensor {self.src_shape}")
        return d_src.data_ptr(), self.n, self.sw, self.sh, self.channels, self.sw * self.channels

    def resize(self, d_src):
        """gms_resize_device into d_dst. Stream-ordered on the context's stream."""
        self.ctx.resize_device(*self._src(d_src), self.d_dst.data_ptr(), self.dw, self.dh, self.dw * self.channels)
        return self.d_dst

    def warp_affine(self, d_src):
        """gms_warp_affine_device by d_M into d_dst. Stream-ordered on the context's stream."""
        self.ctx.warp_affine_device(*self._src(d_src), self.d_M.data_ptr(), self.n_matrices, self.d_dst.data_ptr(), self.dw, self.dh,
                                    self.dw * self.channels)
        return self.d_dst


def _warp_stack(images):
    """-> (device tensor [n, H, W] or [n, H, W, 3], contiguous; whether the caller gave a device tensor)."""
    on_dev = torch.is_tensor(images)
    d = images if on_dev else torch.from_numpy(np.ascontiguousarray(images, dtype=np.uint8))
    if d.dtype != torch.uint8 or d.dim() not in (3, 4) or (d.dim() == 4 and d.shape[3] != 3) or d.numel() == 0:
        raise ValueError("images: uint8 [n, H, W] or [n, H, W, 3]")
    return (d if on_dev else d.cuda()).contiguous(), on_dev


def resize_images(images, dsize, ctx=None):
    """cv::resize(INTER_LINEAR) of n images in one gms_resize_device run. images: uint8 [n, H, W] or [n, H, W, 3], a host array or a
    device tensor; dsize = (width, height). Returns the same kind."""
    from .api import default_context
    ctx = ctx or default_context()
    d, on_dev = _warp_stack(images)
    run = Warp(ctx, d.shape[0], (d.shape[2], d.shape[1]), dsize, 1 if d.dim() == 3 else 3, device=d.device)
    run.resize(d)
    ctx.synchronize()
    return run.d_dst if on_dev else run.d_dst.cpu().numpy()


def warp_affine_images(images, M, dsize, ctx=None):
    """cv::warpAffine(INTER_LINEAR, BORDER_CONSTANT 0) of n images in one gms_warp_affine_device run. M: forward matrices, one ([6],
    [2, 3], [1, 6]) for all images or one per image ([n, 6], [n, 2, 3]); dsize = (width, height). Returns what it was given: host
    array or device tensor."""
    from .api import default_context
    ctx = ctx or default_context()
    d, on_dev = _warp_stack(images)
    m = np.ascontiguousarray(M, dtype=np.float64).reshape(-1, 6)
    run = Warp(ctx, d.shape[0], (d.shape[2], d.shape[1]), dsize, 1 if d.dim() == 3 else 3, n_matrices=len(m), device=d.device)
    run.set_matrices(m)
    torch.cuda.synchronize(d.device)
    run.warp_affine(d)
    ctx.synchronize()
    return run.d_dst if on_dev else run.d_dst.cpu().numpy()


class Rectify:
    """Device buffers of gms_rectify_device for n images of one size and channel count (1: [n, H, W]; 3: [n, H, W, 3]): the rectified
    images d_dst, the valid planes d_valid [n, H', W'] and the plans d_plans (RECTIFY_PLAN_DTYPE bytes; n_plans 1: one for all
    images, or n), sized once, so that run() can be repeated or captured into a graph. The kernel reads d_plans when it runs: a
    captured graph follows set_plans(). camera: a CAMERA_DTYPE record (types.make_camera), the source camera of every image."""

    def __init__(self, ctx, n, src_size, dst_size, camera, channels=1, n_plans=1, device=None):
        self.ctx, self.n, self.channels, self.n_plans = ctx, int(n), int(channels), int(n_plans)
        (self.sw, self.sh), (self.dw, self.dh) = (int(v) for v in src_size), (int(v) for v in dst_size)
        if self.channels not in (1, 3) or self.n < 1 or min(self.sw, self.sh, self.dw, self.dh) < 1 or self.n_plans not in (1, self.n):
            raise ValueError("Rectify: channels 1 or 3, n >= 1, positive sizes, n_plans 1 or n")
        self.camera = np.ascontiguousarray(camera, dtype=CAMERA_DTYPE).reshape(1)
        dev = _device(ctx, device)
        tail = () if self.channels == 1 else (3,)
        self.src_shape = (self.n, self.sh, self.sw) + tail
        self.d_dst = torch.zeros((self.n, self.dh, self.dw) + tail, dtype=torch.uint8, device=dev)
        self.d_valid = torch.zeros((self.n, self.dh, self.dw), dtype=torch.uint8, device=dev)
        self.d_plans = torch.zeros((self.n_plans, RECTIFY_PLAN_DTYPE.itemsize), dtype=torch.uint8, device=dev)
        torch.cuda.synchronize(dev)

    def set_plans(self, plans):
        """n_plans RECTIFY_PLAN_DTYPE records (or RectifyPlan objects) on the host -> d_plans (a copy on torch's current stream)."""
        rec = rectify_plan_records(plans)
        if len(rec) != self.n_plans:
            raise ValueError(f"plans: {self.n_plans} records")
        self.d_plans.copy_(torch.from_numpy(rec.view(np.uint8).reshape(self.n_plans, -1)))

    def run(self, d_src, which):
        """gms_rectify_device of camera `which` (1 or 2) by d_plans into d_dst and d_valid. Stream-ordered on the context's stream."""
        if d_src.dtype != torch.uint8 or tuple(d_src.shape) != self.src_shape or not d_src.is_contiguous():
            raise ValueError(f"images: a contiguous uint8 device tensor {self.src_shape}")
        self.ctx.rectify_device(self.camera, d_src.data_ptr(), self.n, self.sw, self.sh, self.channels, self.sw * self.channels,
                                self.d_plans.data_ptr(), self.n_plans, which, self.d_dst.data_ptr(), self.dw, self.dh,
                                self.dw * self.channels, self.d_valid.data_ptr())
        return self.d_dst


class DensePairs:
    """Device buffers of gms_dense_pairs_device for n pairs of one image size (channels 1: [n, H, W] grey; 3: [n, H, W, 3] BGR) and one
    rectified size: the workspace, the two-view records d_tv (TWO_VIEW_DTYPE bytes; the stage reads R, t and status), the plans, the
    rectified images d_rect1 / d_rect2 (grey), d_color (BGR input: camera 1's rectified colour image), d_valid, d_disp16 and the
    cloud (d_xyz [n, cap, 3], d_cloud_color [n, cap, channels], d_pixel [n, cap], d_count [n]), sized once, so that run() can be
    repeated or captured into a graph; it is one stream with no parallel branches. The kernels read d_tv when they run: a captured
    graph follows set_two_view(). d_tv may also be the tensor a two-view stage writes (pass d_tv=). With a registration
    (set_registration) the points are in the world frame. speckle = (max_speckle_size, max_diff16): gms_dense_pairs_filtered_device,
    the speckle filter on d_disp16 between the matcher and the cloud, and d_removed int32 [n]; None: gms_dense_pairs_device.
    views= (a device view array: SfmRegister.d_views, SfmBundle.d_views_out or any SFM_VIEW_DTYPE bytes) with pose_records= (a
    SfmPairPoses over the same n pairs, or its (d_tv, d_reg, d_pairs) tensors -- the cloud kernel reads each pair's frame_a from the
    pair table): the stage rectifies by those records and puts its
    clouds into the frame of those views -- the pose of pair i is whatever the records hold when run() runs, so a captured graph
    follows SfmPairPoses.run(). Pair i is then the i-th pair of the SfmPairPoses, matched sparsely or not. Without the two, nothing
    changes."""

    def __init__(self, ctx, n, src_size, out_size, camera, dist=None, channels=1, cap=None, min_disp16=16, params=None, device=None, d_tv=None,
                 speckle=None, views=None, pose_records=None):
        from .api import dense_sgm_params, _speckle_pair
        if (views is None) != (pose_records is None):
            raise ValueError("DensePairs: views= and pose_records= go together")
        posed = None
        if pose_records is not None:
            if d_tv is not None:
                raise ValueError("DensePairs: pose_records= brings its own two-view records; d_tv= is the other route")
            posed = _pose_records(pose_records, views, n)
            d_tv = posed[0]
        self.ctx, self.n, self.channels, self.min_disp16 = ctx, int(n), int(channels), int(min_disp16)
        self.speckle = None if speckle is None else _speckle_pair(speckle, "DensePairs")
        (self.sw, self.sh), (self.ow, self.oh) = (int(v) for v in src_size), (int(v) for v in out_size)
        self.camera = make_camera(camera, dist) if not isinstance(camera, np.ndarray) or camera.dtype != CAMERA_DTYPE else camera
        self.params = dense_sgm_params(params)
        self.cap = self.ow * self.oh if cap is None else int(cap)
        ws_bytes = ctx.dense_pairs_workspace_bytes if self.speckle is None else ctx.dense_pairs_filtered_workspace_bytes
        self.ws_bytes = ws_bytes(self.sw, self.sh, self.channels, self.ow, self.oh, self.n, self.params)
        if self.ws_bytes == 0:
            raise GmsError(GMS_ERR_BAD_ARG, "DensePairs: sizes, channels or matcher parameters outside what gms_dense_pairs_device accepts")
        dev = _device(ctx, device)
        z = lambda shape, dt: torch.zeros(shape, dtype=dt, device=dev)
        self.src_shape = (self.n, self.sh, self.sw) + (() if self.channels == 1 else (3,))
        self.d_ws = z((self.ws_bytes,), torch.uint8)
        self.d_tv = d_tv if d_tv is not None else z((self.n, TWO_VIEW_DTYPE.itemsize), torch.uint8)
        self.d_plans = z((self.n, RECTIFY_PLAN_DTYPE.itemsize), torch.uint8)
        self.d_rect1, self.d_rect2, self.d_valid = (z((self.n, self.oh, self.ow), torch.uint8) for _ in range(3))
        self.d_color = z((self.n, self.oh, self.ow, 3), torch.uint8) if self.channels == 3 else None
        self.d_disp16 = z((self.n, self.oh, self.ow), torch.int16)
        k = max(self.cap, 1)
        self.d_xyz, self.d_cloud_color = z((self.n, k, 3), torch.float32), z((self.n, k, self.channels), torch.uint8)
        self.d_pixel, self.d_count = z((self.n, k), torch.int32), z((self.n,), torch.int32)
        self.d_removed = None if self.speckle is None else z((self.n,), torch.int32)
        self.reg = None
        if posed is not None:
            self.set_registration(posed[2], posed[1], views, posed[3])
        torch.cuda.synchronize(dev)

    def set_two_view(self, two_view):
        """n TWO_VIEW_DTYPE records on the host -> d_tv (a copy on torch's current stream)."""
        rec = np.ascontiguousarray(two_view, dtype=TWO_VIEW_DTYPE).reshape(self.n)
        self.d_tv.copy_(torch.from_numpy(rec.view(np.uint8).reshape(self.n, -1)))

    def set_registration(self, d_pairs, d_reg, d_views, n_frames):
        """The device tensors of the pairs (PAIR_DTYPE), their registration (SFM_PAIR_REG_DTYPE) and the views (SFM_VIEW_DTYPE) as
        SfmRegister leaves them; None, None, None, 0 for camera 1's frame."""
        self.reg = None if d_pairs is None else (d_pairs, d_reg, d_views, int(n_frames))

    def plans(self):
        """The plans of the last run, RECTIFY_PLAN_DTYPE [n] on the host (synchronises)."""
        return self.d_plans.cpu().numpy().reshape(-1).view(RECTIFY_PLAN_DTYPE).copy()

    def run(self, d_img1, d_img2):
        """gms_dense_pairs_device. Stream-ordered on the context's stream; no allocation, no synchronisation."""
        for d in (d_img1, d_img2):
            if d.dtype != torch.uint8 or tuple(d.shape) != self.src_shape or not d.is_contiguous():
                raise ValueError(f"images: contiguous uint8 device tensors {self.src_shape}")
        reg = {} if self.reg is None else dict(d_pairs=self.reg[0].data_ptr(), d_reg=self.reg[1].data_ptr(), d_views=self.reg[2].data_ptr(),
                                               n_frames=self.reg[3])
        args = (self.camera, self.params, d_img1.data_ptr(), d_img2.data_ptr(), self.n, self.sw, self.sh, self.channels, self.d_tv.data_ptr(),
                self.ow, self.oh, self.min_disp16, self.d_ws.data_ptr(), self.ws_bytes, self.d_plans.data_ptr(), self.d_rect1.data_ptr(),
                self.d_rect2.data_ptr(), self.d_valid.data_ptr(), None if self.d_color is None else self.d_color.data_ptr(),
                self.d_disp16.data_ptr(), self.cap, self.d_xyz.data_ptr(), self.d_cloud_color.data_ptr(), self.d_pixel.data_ptr(),
                self.d_count.data_ptr())
        if self.speckle is None:
            self.ctx.dense_pairs_device(*args, **reg)
        else:
            self.ctx.dense_pairs_filtered_device(*args, self.speckle[0], self.speckle[1], self.d_removed.data_ptr(), **reg)
        return self.d_count


class SpeckleFilter:
    """The workspace of gms_filter_speckles_device for n int16 maps of one size (w, h), and d_removed int32 [n], sized once, so that
    run() can be repeated or captured into a graph; it is one stream with no parallel branches."""

    def __init__(self, ctx, n, size, device=None):
        self.ctx, self.n = ctx, int(n)
        self.width, self.height = (int(v) for v in size)
        self.ws_bytes = ctx.filter_speckles_workspace_bytes(self.width, self.height, self.n)
        if self.ws_bytes == 0:
            raise GmsError(GMS_ERR_BAD_ARG, "SpeckleFilter: width, height 1..8192 and n 1..65535")
        dev = _device(ctx, device)
        self.d_ws = torch.zeros((self.ws_bytes,), dtype=torch.uint8, device=dev)
        self.d_removed = torch.zeros((self.n,), dtype=torch.int32, device=dev)
        torch.cuda.synchronize(dev)

    def run(self, d_disp16, new_val, max_speckle_size, max_diff):
        """filterSpeckles on d_disp16, a contiguous int16 device tensor [n, height, width], in place; the pixels changed per map in
        d_removed. Stream-ordered on the context's stream; no allocation, no synchronisation."""
        if d_disp16.dtype != torch.int16 or tuple(d_disp16.shape) != (self.n, self.height, self.width) or not d_disp16.is_contiguous():
            raise ValueError(f"d_disp16: a contiguous int16 device tensor {(self.n, self.height, self.width)}")
        self.ctx.filter_speckles_device(d_disp16.data_ptr(), self.n, self.width, self.height, new_val, max_speckle_size, max_diff,
                                        self.d_ws.data_ptr(), self.ws_bytes, self.d_removed.data_ptr())
        return d_disp16


def filter_speckles_batch(maps, new_val, max_speckle_size, max_diff, ctx=None, return_removed=False):
    """filterSpeckles for n maps in one gms_filter_speckles_device run. maps: int16 [n, H, W]; a host array gives new host arrays, a
    contiguous device tensor is filtered in place and returned. return_removed=True: also the int32 [n] counts of pixels changed."""
    from .api import default_context
    ctx = ctx or default_context()
    on_dev = isinstance(maps, torch.Tensor)
    if on_dev:
        d = maps
        if d.dtype != torch.int16 or d.dim() != 3 or not d.is_contiguous():
            raise ValueError("maps: a contiguous int16 device tensor [n, H, W]")
    else:
        m = np.asarray(maps)
        if m.dtype != np.int16 or m.ndim != 3 or m.size == 0:
            raise ValueError("maps: int16 [n, H, W]")
        d = torch.from_numpy(np.ascontiguousarray(m)).cuda()
    n, h, w = d.shape
    run = SpeckleFilter(ctx, n, (w, h), d.device)
    run.run(d, new_val, max_speckle_size, max_diff)
    ctx.synchronize()
    out = d if on_dev else d.cpu().numpy()
    removed = run.d_removed if on_dev else run.d_removed.cpu().numpy()
    return (out, removed) if return_removed else out


def dense_fuse_sources(run, frame_a=None):
    """The n fusion sources of a DensePairs run, as dicts of views into its device tensors (nothing is copied): d_disp16, d_valid,
    d_plan, d_xyz, d_color, d_count, filtered16, min_disp16, and with a registration d_view (the view of the pair's frame_a) and d_reg.
    frame_a: the pairs' frame_a on the host; default: read from the run's pair table (one readback, when the table is built)."""
    f16 = (int(np.asarray(run.params).reshape(-1)[0]["min_disparity"]) - 1) * 16
    if run.reg is not None and frame_a is None:
        frame_a = run.reg[0].cpu().numpy().reshape(-1).view(PAIR_DTYPE)["frame_a"]
    out = []
    for j in range(run.n):
        s = dict(d_disp16=run.d_disp16[j], d_valid=run.d_valid[j], d_plan=run.d_plans[j], d_xyz=run.d_xyz[j], d_color=run.d_cloud_color[j],
                 d_count=run.d_count[j:j + 1], filtered16=f16, min_disp16=run.min_disp16, cap=run.cap)
        if run.reg is not None:
            a = int(frame_a[j])
            if not 0 <= a < run.reg[3]:
                raise ValueError("dense_fuse_sources: a pair's frame_a is not a frame of the registration")
            s.update(d_view=run.reg[2].reshape(run.reg[3], -1)[a], d_reg=run.reg[1].reshape(run.n, -1)[j])
        out.append(s)
    return out


class DenseFuse:
    """Device buffers of gms_dense_fuse_device: the source table and the neighbour table, built and uploaded once,
    the workspace and the fused cloud (d_xyz [fused_cap, 3], d_color [fused_cap, channels], d_source, d_index, d_support, d_conflict,
    d_counts [n_src + 1]), so that run() can be repeated or captured into a graph; it is one stream with no parallel branches. The
    table holds pointers into the sources' tensors, which this object keeps alive: the kernels read maps, plans, points, counts, views
    and scales when they run, so a run -- or a captured graph -- follows whatever the dense stage and the registration wrote there
    since. sources: DensePairs objects (every pair of the run, in order) and / or dicts as dense_fuse_sources returns them -- device
    tensors d_disp16 int16 [H, W], d_valid uint8 [H, W], d_plan (200 bytes), d_xyz float32 [cap, 3], d_count int32 [1]; optional
    d_color uint8 [cap, channels], d_view (an SFM_VIEW_DTYPE record's bytes; default identity), d_reg (SFM_PAIR_REG_DTYPE; default
    S = 1, ok), cap (default d_xyz's rows), filtered16 (default -16), min_disp16 (default 16).
    neighbors: types.dense_fuse_neighbors' table; default every other source, which needs at most 33 sources (ValueError beyond). For
    j > i the table should list i for j whenever it lists j for i: a one-sided entry lets duplicates survive."""

    def __init__(self, ctx, sources, neighbors=None, channels=1, tol16=16, min_support=1, fused_cap=None, device=None):
        self.ctx, self.channels, self.tol16, self.min_support = ctx, int(channels), int(tol16), int(min_support)
        self.sources = []
        for s in sources:
            self.sources += dense_fuse_sources(s) if isinstance(s, DensePairs) else [s]
        self.n = len(self.sources)
        if self.n < 1:
            raise ValueError("DenseFuse: at least one source")
        nb = dense_fuse_neighbors(self.n, neighbors)
        tab = np.zeros(self.n, DENSE_FUSE_SRC_DTYPE)
        sizes = dict(d_plan=RECTIFY_PLAN_DTYPE.itemsize, d_view=SFM_VIEW_DTYPE.itemsize, d_reg=SFM_PAIR_REG_DTYPE.itemsize)
        for i, s in enumerate(self.sources):
            d, v, xyz = s["d_disp16"], s["d_valid"], s["d_xyz"]
            if d.dtype != torch.int16 or d.dim() != 2 or v.dtype != torch.uint8 or v.shape != d.shape or xyz.dtype != torch.float32 or \
                    xyz.dim() != 2 or xyz.shape[1] != 3 or s["d_count"].dtype != torch.int32 or not all(t.is_contiguous() for t in (d, v, xyz)):
                raise ValueError("DenseFuse: d_disp16 int16 [H, W], d_valid uint8 [H, W], d_xyz float32 [cap, 3], d_count int32, contiguous")
            col = s.get("d_color")
            if col is not None and (col.dtype != torch.uint8 or not col.is_contiguous() or col.numel() < xyz.shape[0] * self.channels):
                raise ValueError("DenseFuse: d_color uint8 [cap, channels], contiguous")
            for name, size in sizes.items():
                t = s.get(name)
                if t is not None and (t.dtype != torch.uint8 or not t.is_contiguous() or t.numel() != size):
                    raise ValueError(f"DenseFuse: {name}: the record's {size} bytes as a contiguous uint8 tensor")
            if s.get("d_plan") is None:
                raise ValueError("DenseFuse: d_plan")
            for name in DENSE_FUSE_SRC_DTYPE.names[:8]:
                tab[name][i] = 0 if s.get(name) is None else s[name].data_ptr()
            tab["width"][i], tab["height"][i], tab["cap"][i] = d.shape[1], d.shape[0], int(s.get("cap", xyz.shape[0]))
            if tab["cap"][i] > xyz.shape[0]:
                raise ValueError("DenseFuse: cap exceeds d_xyz's rows")
            tab["filtered16"][i], tab["min_disp16"][i] = int(s.get("filtered16", -16)), int(s.get("min_disp16", 16))
        self.table = tab
        self.max_cap = max(int(tab["cap"].max()), 1)
        self.fused_cap = int(tab["cap"].astype(np.int64).sum()) if fused_cap is None else int(fused_cap)
        self.ws_bytes = ctx.dense_fuse_workspace_bytes(self.n, self.max_cap)
        if self.ws_bytes == 0 or self.fused_cap < 0 or self.fused_cap > 2 ** 31 - 1:
            raise GmsError(GMS_ERR_BAD_ARG, "DenseFuse: the number of sources, their caps or fused_cap outside what gms_dense_fuse_device accepts")
        dev = _device(ctx, device)
        z = lambda shape, dt: torch.zeros(shape, dtype=dt, device=dev)
        k = max(self.fused_cap, 1)
        self.d_ws = z((self.ws_bytes,), torch.uint8)
        self.d_src = _to_dev(tab, dev)
        self.d_neighbors, self.n_nb = torch.from_numpy(nb).to(dev), nb.shape[1]
        self.d_xyz, self.d_color = z((k, 3), torch.float32), z((k, self.channels), torch.uint8)
        self.d_source, self.d_index = z((k,), torch.int32), z((k,), torch.int32)
        self.d_support, self.d_conflict = z((k,), torch.uint8), z((k,), torch.uint8)
        self.d_counts = z((self.n + 1,), torch.int32)
        torch.cuda.synchronize(dev)

    def run(self):
        """gms_dense_fuse_device. Stream-ordered on the context's stream; no allocation, no synchronisation."""
        self.ctx.dense_fuse_device(self.d_src.data_ptr(), self.n, self.max_cap, self.d_neighbors.data_ptr(), self.n_nb, self.channels, self.tol16,
                                   self.min_support, self.d_ws.data_ptr(), self.ws_bytes, self.fused_cap, self.d_xyz.data_ptr(),
                                   self.d_color.data_ptr(), self.d_source.data_ptr(), self.d_index.data_ptr(), self.d_support.data_ptr(),
                                   self.d_conflict.data_ptr(), self.d_counts.data_ptr())
        return self.d_counts

    def result(self):
        """Waits for the context's stream -> the fused cloud on the host: points float32 [k, 3], colors uint8 [k] or [k, 3], source,
        index int32 [k], support, conflict uint8 [k] with k = min(total, fused_cap), and counts int32 [n_src + 1]."""
        self.ctx.synchronize()
        counts = self.d_counts.cpu().numpy()
        k = min(int(counts[-1]), self.fused_cap)
        colors = self.d_color[:k].cpu().numpy()
        return dict(points=self.d_xyz[:k].cpu().numpy(), colors=colors if self.channels == 3 else colors[:, 0],
                    source=self.d_source[:k].cpu().numpy(), index=self.d_index[:k].cpu().numpy(), support=self.d_support[:k].cpu().numpy(),
                    conflict=self.d_conflict[:k].cpu().numpy(), counts=counts)


def fuse_dense(ctx, runs, neighbors=None, channels=1, tol16=16, min_support=1, fused_cap=None, device=None):
    """One fused cloud from the outputs of the dense stage: `runs` holds DensePairs objects that have run (all their pairs, run after
    run, are the sources) or equivalent dicts (DenseFuse). Builds a DenseFuse, runs it once and returns its result()."""
    job = DenseFuse(ctx, runs, neighbors, channels, tol16, min_support, fused_cap, device)
    torch.cuda.synchronize(job.d_ws.device)
    job.run()
    return job.result()


class ChessCorners:
    """Device buffers of gms_chess_candidates_device for n grey images of one size: the workspace, the candidate records
    [n, max_candidates] and the counts [n], sized once, so that run() can be repeated or captured into a graph on new pixels in the
    same tensor. candidates() reads the records back (the only readback of the corner search)."""

    def __init__(self, ctx, n, width, height, max_candidates=256, device=None):
        self.ctx, self.n, self.width, self.height, self.max_candidates = ctx, int(n), int(width), int(height), int(max_candidates)
        self.ws_bytes = ctx.chess_candidates_workspace_bytes(width, height, n)
        if self.ws_bytes == 0 or not 1 <= self.max_candidates <= 4096:
            raise ValueError("ChessCorners: image size, batch size or max_candidates rejected (include/gms.h)")
        dev = _device(ctx, device)
        self.d_ws = torch.zeros(self.ws_bytes, dtype=torch.uint8, device=dev)
        self.d_out = torch.zeros(self.n * self.max_candidates * 12, dtype=torch.uint8, device=dev)
        self.d_counts = torch.zeros(self.n, dtype=torch.int32, device=dev)
        torch.cuda.synchronize(dev)

    def run(self, d_images):
        """gms_chess_candidates_device on a contiguous uint8 device tensor [n, H, W]. Stream-ordered on the context's stream."""
        if d_images.dtype != torch.uint8 or tuple(d_images.shape) != (self.n, self.height, self.width) or not d_images.is_contiguous():
            raise ValueError(f"images: a contiguous uint8 device tensor {(self.n, self.height, self.width)}")
        self.ctx.chess_candidates_device(d_images.data_ptr(), self.n, self.width, self.height, self.max_candidates, self.d_ws.data_ptr(),
                                         self.ws_bytes, self.d_out.data_ptr(), self.d_counts.data_ptr())

    def candidates(self):
        """Waits for the context's stream -> one CHESS_CANDIDATE_DTYPE array per image (its first counts[i] records)."""
        from .types import CHESS_CANDIDATE_DTYPE
        self.ctx.synchronize()
        counts = self.d_counts.cpu().numpy()
        recs = self.d_out.cpu().numpy().view(CHESS_CANDIDATE_DTYPE).reshape(self.n, self.max_candidates)
        return [recs[i, :int(counts[i])].copy() for i in range(self.n)]


def corner_subpix_images(ctx, d_images, image_of, corners, max_iter=30, eps=0.1):
    """gms_corner_subpix_device: corners float64 [m, 2] (host) of images d_images[image_of[k]] -> (refined [m, 2], status [m]) on the
    host; the images stay on the device."""
    n, h, w = d_images.shape
    pts = np.ascontiguousarray(corners, dtype=np.float64).reshape(-1, 2)
    if len(pts) == 0:
        return pts, np.zeros(0, np.int32)
    dev = d_images.device
    d_pts = torch.from_numpy(pts).to(dev)
    d_of = torch.from_numpy(np.ascontiguousarray(image_of, dtype=np.int32)).to(dev)
    d_status = torch.zeros(len(pts), dtype=torch.int32, device=dev)
    torch.cuda.synchronize(dev)
    ctx.corner_subpix_device(d_images.data_ptr(), n, w, h, d_of.data_ptr(), d_pts.data_ptr(), len(pts), 5, max_iter, eps, d_status.data_ptr())
    ctx.synchronize()
    return d_pts.cpu().numpy(), d_status.cpu().numpy()


class SfmRegister:
    """Device buffers of one gms_sfm_register_device call over a fixed pair list: the frame offsets, the pair table, its plan
    (api.sfm_plan, computed here on the host from the pair list), the workspace and every output, sized once, so that run() can be
    repeated or captured into a graph. The inputs -- survivors, mask, points and two-view records, as gms_two_view_batch_device
    leaves them -- are either the caller's device tensors, handed to run(), or the object's own (load() copies host arrays into them;
    run() without arguments reads them). frame_off: int64 [n_frames + 1] on the host; pairs: PAIR_DTYPE records.
    keep: None -- gms_sfm_register_device; a uint8 device tensor with one byte per match slot (a MatchUnique's d_keep)
    -- every run() is gms_sfm_register_keep_device on it; True -- the same on the object's own plane, which load(..., keep=) fills."""

    def __init__(self, ctx, frame_off, pairs, root=0, min_links=8, cloud_cap=None, device=None, d_frame_off=None, d_pairs=None, keep=None):
        from .api import sfm_plan
        from .types import SFM_PAIR_REG_DTYPE, SFM_SUMMARY_DTYPE, SFM_VIEW_DTYPE, TWO_VIEW_DTYPE
        self.d_keep = None if keep is None or keep is False or keep is True else keep   # (True: the object's own, made below)
        self.ctx, self.root, self.min_links = ctx, int(root), int(min_links)
        self.frame_off = np.ascontiguousarray(frame_off, dtype=np.int64)
        self.recs = np.ascontiguousarray(pairs, dtype=PAIR_DTYPE)
        self.n_frames, self.n_pairs, self.total_kp = len(self.frame_off) - 1, len(self.recs), int(self.frame_off[-1])
        if not 0 <= self.root < self.n_frames or self.min_links < 1:
            raise ValueError("SfmRegister: root is a frame index, min_links at least 1")
        self.plan = sfm_plan(self.recs, self.n_frames, self.root)   # (refuses a frame index out of range)
        n = self.n_pairs
        self.total_m = int((self.recs["match_off"] + np.maximum(self.recs["m"], 0)).max()) if n else 0
        self.max_m = int(self.recs["m"].max()) if n else 0
        self.cloud_cap = max(self.total_kp // 2, 0) if cloud_cap is None else int(cloud_cap)
        self.ws_bytes = ctx.sfm_register_workspace_bytes(self.n_frames, n, self.total_kp, self.total_m)
        if self.ws_bytes == 0:
            raise ValueError("SfmRegister: sizes rejected (include/gms.h)")
        dev = _device(ctx, device)
        self.device = dev
        self.d_frame_off = d_frame_off if d_frame_off is not None else torch.from_numpy(self.frame_off).to(dev)
        self.d_pairs = d_pairs if d_pairs is not None else (_to_dev(self.recs, dev) if n else torch.zeros(24, dtype=torch.uint8, device=dev))
        self.d_plan = _to_dev(self.plan, dev) if n else torch.zeros(16, dtype=torch.uint8, device=dev)
        self.d_ws = torch.zeros(self.ws_bytes, dtype=torch.uint8, device=dev)
        m, cap = max(self.total_m, 1), max(self.cloud_cap, 1)
        self.d_views = torch.zeros(self.n_frames * SFM_VIEW_DTYPE.itemsize, dtype=torch.uint8, device=dev)
        self.d_reg = torch.zeros(max(n, 1) * SFM_PAIR_REG_DTYPE.itemsize, dtype=torch.uint8, device=dev)
        self.d_world = torch.zeros(m * 3, dtype=torch.float64, device=dev)
        self.d_track = torch.zeros(m, dtype=torch.int32, device=dev)
        self.d_cloud = torch.zeros(cap * 3, dtype=torch.float64, device=dev)
        self.d_cloud_id, self.d_cloud_obs, self.d_cloud_est = (torch.zeros(cap, dtype=torch.int32, device=dev) for _ in range(3))
        self.d_cloud_spread = torch.zeros(cap, dtype=torch.float64, device=dev)
        self.d_summary = torch.zeros(SFM_SUMMARY_DTYPE.itemsize, dtype=torch.uint8, device=dev)
        self._own = None
        self._tv_bytes = TWO_VIEW_DTYPE.itemsize
        if keep is True:
            self.d_keep = torch.zeros(m, dtype=torch.uint8, device=dev)
        elif self.d_keep is not None and (self.d_keep.dtype != torch.uint8 or self.d_keep.numel() < self.total_m):
            raise ValueError("SfmRegister: keep is a uint8 tensor with one byte per match slot")
        torch.cuda.synchronize(dev)

    def _own_inputs(self):
        if self._own is None:
            m, n, dev = max(self.total_m, 1), max(self.n_pairs, 1), self.device
            self._own = (torch.zeros(m * 16, dtype=torch.uint8, device=dev), torch.zeros(m, dtype=torch.uint8, device=dev),
                         torch.zeros(m * 3, dtype=torch.float64, device=dev), torch.zeros(n * self._tv_bytes, dtype=torch.uint8, device=dev))
        return self._own

    def load(self, matches, mask, points3d, two_view, keep=None):
        """Host arrays (run_dataset's out, mask, points3d, two_view) into the object's own input tensors (same tensors every time: a
        captured run() reads what the latest load() left). keep: a host keep plane into the object's plane (keep=True or a tensor at
        construction)."""
        from .types import TWO_VIEW_DTYPE
        d_m, d_mask, d_pts, d_tv = self._own_inputs()
        m = np.ascontiguousarray(matches, dtype=DMATCH_DTYPE)
        mk = np.ascontiguousarray(mask, dtype=np.uint8)
        pts = np.ascontiguousarray(points3d, dtype=np.float64).reshape(-1, 3)
        tv = np.ascontiguousarray(two_view, dtype=TWO_VIEW_DTYPE)
        if min(len(m), len(mk), len(pts)) < self.total_m or len(tv) != self.n_pairs:
            raise ValueError("matches, mask and points3d cover every pair's match range; one two_view record per pair")
        if self.total_m:
            d_m[:self.total_m * 16].copy_(torch.from_numpy(m[:self.total_m].view(np.uint8).reshape(-1)))
            d_mask[:self.total_m].copy_(torch.from_numpy(mk[:self.total_m]))
            d_pts[:self.total_m * 3].copy_(torch.from_numpy(pts[:self.total_m].reshape(-1)))
        if self.n_pairs:
            d_tv[:self.n_pairs * self._tv_bytes].copy_(torch.from_numpy(tv.view(np.uint8).reshape(-1)))
        if keep is not None:
            kp = np.ascontiguousarray(keep, dtype=np.uint8)
            if self.d_keep is None or len(kp) < self.total_m:
                raise ValueError("load: a keep plane needs keep=True (or a tensor) at construction, and one byte per match slot")
            if self.total_m:
                self.d_keep[:self.total_m].copy_(torch.from_numpy(kp[:self.total_m]))

    def run(self, d_matches=None, d_mask=None, d_points3d=None, d_tv=None):
        """gms_sfm_register_device (with a keep plane: gms_sfm_register_keep_device), stream-ordered on the context's stream; no
        allocation, no synchronisation, no readback."""
        given = (d_matches, d_mask, d_points3d, d_tv)
        if any(t is None for t in given):
            if not all(t is None for t in given):
                raise ValueError("run: all four input tensors, or none (the object's own)")
            given = self._own_inputs()
        d_matches, d_mask, d_points3d, d_tv = given
        self.ctx.sfm_register_device(self.d_frame_off.data_ptr(), self.n_frames, self.total_kp, self.d_pairs.data_ptr(), self.d_plan.data_ptr(),
                                     self.n_pairs, self.max_m, self.total_m, d_matches.data_ptr(), d_mask.data_ptr(), d_points3d.data_ptr(),
                                     d_tv.data_ptr(), self.root, self.min_links, self.d_ws.data_ptr(), self.ws_bytes, self.d_views.data_ptr(),
                                     self.d_reg.data_ptr(), self.d_world.data_ptr(), self.d_track.data_ptr(), self.cloud_cap,
                                     self.d_cloud.data_ptr(), self.d_cloud_id.data_ptr(), self.d_cloud_obs.data_ptr(),
                                     self.d_cloud_est.data_ptr(), self.d_cloud_spread.data_ptr(), self.d_summary.data_ptr(),
                                     None if self.d_keep is None else self.d_keep.data_ptr())

    def results(self, trim=True):
        """Waits for the context's stream -> dict(plan, views, registration, points_world, track, cloud, cloud_id, cloud_obs, cloud_est,
        cloud_spread, summary) on the host; trim: the cloud arrays cut to the tracks they hold."""
        from .api import sfm_trim
        from .types import SFM_PAIR_REG_DTYPE, SFM_SUMMARY_DTYPE, SFM_VIEW_DTYPE
        self.ctx.synchronize()
        m, cap = self.total_m, self.cloud_cap
        out = dict(plan=self.plan.copy(), views=self.d_views.cpu().numpy().view(SFM_VIEW_DTYPE).copy(),
                   registration=self.d_reg.cpu().numpy().view(SFM_PAIR_REG_DTYPE)[:self.n_pairs].copy(),
                   points_world=self.d_world.cpu().numpy().reshape(-1, 3)[:m].copy(), track=self.d_track.cpu().numpy()[:m].copy(),
                   cloud=self.d_cloud.cpu().numpy().reshape(-1, 3)[:cap].copy(), cloud_id=self.d_cloud_id.cpu().numpy()[:cap].copy(),
                   cloud_obs=self.d_cloud_obs.cpu().numpy()[:cap].copy(), cloud_est=self.d_cloud_est.cpu().numpy()[:cap].copy(),
                   cloud_spread=self.d_cloud_spread.cpu().numpy()[:cap].copy(), summary=self.d_summary.cpu().numpy().view(SFM_SUMMARY_DTYPE).copy())
        return sfm_trim(out) if trim else out


class MatchUnique:
    """Device buffers of one gms_match_unique_device call over a fixed pair list (one-to-one matches per pair): the
    frame offsets, the pair table, the workspace, the keep plane d_keep (uint8 per match slot) and d_counts (int32 live, kept per
    pair), sized once, so that run() can be repeated or captured into a graph. The inputs -- matches, and optionally the mask and the
    two-view records as gms_two_view_batch_device leaves them -- are the caller's device tensors, handed to run(), or the object's
    own (load() copies host arrays into them; run() without arguments reads them). Any pair list: no plan is made. total_m: the match
    arrays' length, where it is more than the pairs' ranges need (the plane then has that many bytes)."""

    def __init__(self, ctx, frame_off, pairs, device=None, d_frame_off=None, d_pairs=None, total_m=None):
        from .types import TWO_VIEW_DTYPE
        self.ctx = ctx
        self.frame_off = np.ascontiguousarray(frame_off, dtype=np.int64)
        self.recs = np.ascontiguousarray(pairs, dtype=PAIR_DTYPE)
        self.n_frames, self.n_pairs, self.total_kp = len(self.frame_off) - 1, len(self.recs), int(self.frame_off[-1])
        n = self.n_pairs
        self.total_m = int((self.recs["match_off"] + np.maximum(self.recs["m"], 0)).max()) if n else 0
        self.total_m = max(self.total_m, 0 if total_m is None else int(total_m))
        self.max_m = int(self.recs["m"].max()) if n else 0
        self.ws_bytes = ctx.match_unique_workspace_bytes(n, self.total_kp, self.total_m) if self.n_frames >= 1 else 0
        if self.ws_bytes == 0:
            raise ValueError("MatchUnique: sizes rejected (include/gms.h)")
        dev = _device(ctx, device)
        self.device = dev
        self.d_frame_off = d_frame_off if d_frame_off is not None else torch.from_numpy(self.frame_off).to(dev)
        self.d_pairs = d_pairs if d_pairs is not None else (_to_dev(self.recs, dev) if n else torch.zeros(24, dtype=torch.uint8, device=dev))
        self.d_ws = torch.zeros(self.ws_bytes, dtype=torch.uint8, device=dev)
        self.d_keep = torch.zeros(max(self.total_m, 1), dtype=torch.uint8, device=dev)
        self.d_counts = torch.zeros(2 * max(n, 1), dtype=torch.int32, device=dev)
        self._own = None
        self._own_mask = self._own_tv = False
        self._tv_bytes = TWO_VIEW_DTYPE.itemsize
        torch.cuda.synchronize(dev)

    def load(self, matches, mask=None, two_view=None):
        """Host arrays into the object's own input tensors (same tensors every time: a captured run() reads what the latest load()
        left). Whether a mask and two-view records take part is fixed by the first load()."""
        from .types import TWO_VIEW_DTYPE
        m = np.ascontiguousarray(matches, dtype=DMATCH_DTYPE)
        if self._own is None:
            mm, n, dev = max(self.total_m, 1), max(self.n_pairs, 1), self.device
            self._own = (torch.zeros(mm * 16, dtype=torch.uint8, device=dev), torch.zeros(mm, dtype=torch.uint8, device=dev),
                         torch.zeros(n * self._tv_bytes, dtype=torch.uint8, device=dev))
            self._own_mask, self._own_tv = mask is not None, two_view is not None
        if (mask is not None) != self._own_mask or (two_view is not None) != self._own_tv:
            raise ValueError("load: with a mask / two-view records every time, or never")
        if len(m) < self.total_m or (mask is not None and len(mask) < self.total_m) or (two_view is not None and len(two_view) != self.n_pairs):
            raise ValueError("matches and mask cover every pair's match range; one two_view record per pair")
        d_m, d_mask, d_tv = self._own
        if self.total_m:
            d_m[:self.total_m * 16].copy_(torch.from_numpy(m[:self.total_m].view(np.uint8).reshape(-1)))
            if mask is not None:
                d_mask[:self.total_m].copy_(torch.from_numpy(np.ascontiguousarray(mask, dtype=np.uint8)[:self.total_m]))
        if self.n_pairs and two_view is not None:
            d_tv[:self.n_pairs * self._tv_bytes].copy_(torch.from_numpy(np.ascontiguousarray(two_view, dtype=TWO_VIEW_DTYPE).view(np.uint8).reshape(-1)))

    def run(self, d_matches=None, d_mask=None, d_tv=None):
        """gms_match_unique_device, stream-ordered on the context's stream; no allocation, no synchronisation, no readback. d_matches
        None: the object's own inputs."""
        if d_matches is None:
            if self._own is None or d_mask is not None or d_tv is not None:
                raise ValueError("run: the caller's tensors, or none after a load() (the object's own)")
            d_matches, d_mask, d_tv = self._own[0], self._own[1] if self._own_mask else None, self._own[2] if self._own_tv else None
        self.ctx.match_unique_device(self.d_frame_off.data_ptr(), self.n_frames, self.total_kp, self.d_pairs.data_ptr(), self.n_pairs, self.max_m,
                                     self.total_m, d_matches.data_ptr(), None if d_mask is None else d_mask.data_ptr(),
                                     None if d_tv is None else d_tv.data_ptr(), self.d_ws.data_ptr(), self.ws_bytes, self.d_keep.data_ptr(),
                                     self.d_counts.data_ptr())

    def results(self):
        """Waits for the context's stream -> (keep uint8 [total_m], counts int32 [n_pairs, 2] = live, kept) on the host."""
        self.ctx.synchronize()
        return self.d_keep.cpu().numpy()[:self.total_m].copy(), self.d_counts.cpu().numpy().reshape(-1, 2)[:self.n_pairs].copy()


def unique_matches(ctx, frame_off, pairs, matches, mask=None, two_view=None, device=None):
    """The convenience call: host arrays of many pairs' matches (and optionally the two-view stage's mask and records) ->
    MatchUnique.results() after one gms_match_unique_device run."""
    job = MatchUnique(ctx, frame_off, pairs, device)
    job.load(matches, mask, two_view)
    torch.cuda.synchronize(job.device)
    job.run()
    return job.results()


class SfmBundle:
    """Device buffers of one gms_sfm_ba_device call (bundle adjustment behind the registration) over a fixed pair list
    and cloud capacity: the workspace and the outputs, sized once, so that run() can be repeated or captured into a graph. The inputs
    are either device tensors handed to run() -- a SfmRegister's own (`after`) and the keypoints, survivors and mask the two-view
    stage read and left -- or the object's own, which load() fills from host arrays. camera = (fx, fy, cx, cy), dist = (k1, k2, p1,
    p2, k3) or None; ba: n_iters, n_cg, lambda0, cg_tol, ftol, huber_px, retriangulate."""

    def __init__(self, ctx, frame_off, pairs, cloud_cap, camera, dist=None, device=None, d_frame_off=None, d_pairs=None, **ba):
        from .types import SFM_BA_SUMMARY_DTYPE, SFM_VIEW_DTYPE, make_camera, sfm_ba_params
        self.ctx = ctx
        self.frame_off = np.ascontiguousarray(frame_off, dtype=np.int64)
        self.recs = np.ascontiguousarray(pairs, dtype=PAIR_DTYPE)
        self.n_frames, self.n_pairs, self.total_kp = len(self.frame_off) - 1, len(self.recs), int(self.frame_off[-1])
        n = self.n_pairs
        self.total_m = int((self.recs["match_off"] + np.maximum(self.recs["m"], 0)).max()) if n else 0
        self.cloud_cap = int(cloud_cap)
        self.camera, self.params = make_camera(camera, dist), sfm_ba_params(**ba)
        self.ws_bytes = ctx.sfm_ba_workspace_bytes(self.n_frames, n, self.total_kp, self.cloud_cap)
        if self.ws_bytes == 0:
            raise ValueError("SfmBundle: sizes rejected (include/gms.h)")
        dev = _device(ctx, device)
        self.device = dev
        self.d_frame_off = d_frame_off if d_frame_off is not None else torch.from_numpy(self.frame_off).to(dev)
        self.d_pairs = d_pairs if d_pairs is not None else (_to_dev(self.recs, dev) if n else torch.zeros(24, dtype=torch.uint8, device=dev))
        self.d_ws = torch.zeros(self.ws_bytes, dtype=torch.uint8, device=dev)
        cap = max(self.cloud_cap, 1)
        self.d_views_out = torch.zeros(self.n_frames * SFM_VIEW_DTYPE.itemsize, dtype=torch.uint8, device=dev)
        self.d_cloud_out = torch.zeros(cap * 3, dtype=torch.float64, device=dev)
        self.d_status = torch.zeros(cap, dtype=torch.int32, device=dev)
        self.d_summary = torch.zeros(SFM_BA_SUMMARY_DTYPE.itemsize, dtype=torch.uint8, device=dev)
        self._own = None
        torch.cuda.synchronize(dev)

    def _own_inputs(self):
        from .types import SFM_PAIR_REG_DTYPE, SFM_SUMMARY_DTYPE, SFM_VIEW_DTYPE
        if self._own is None:
            m, n, cap, dev = max(self.total_m, 1), max(self.n_pairs, 1), max(self.cloud_cap, 1), self.device
            u8 = dict(dtype=torch.uint8, device=dev)
            self._own = dict(kp=torch.zeros(max(self.total_kp, 1) * 28, **u8), matches=torch.zeros(m * 16, **u8), mask=torch.zeros(m, **u8),
                             views=torch.zeros(self.n_frames * SFM_VIEW_DTYPE.itemsize, **u8), reg=torch.zeros(n * SFM_PAIR_REG_DTYPE.itemsize, **u8),
                             track=torch.zeros(m, dtype=torch.int32, device=dev), cloud=torch.zeros(cap * 3, dtype=torch.float64, device=dev),
                             cloud_id=torch.zeros(cap, dtype=torch.int32, device=dev), summary=torch.zeros(SFM_SUMMARY_DTYPE.itemsize, **u8))
        return self._own

    def load(self, keypoints, matches, mask, registration):
        """Host arrays into the object's own input tensors (the same tensors every time: a captured run() reads what the latest load()
        left). registration: SfmRegister.results() / registerViews' dict, trimmed or not."""
        from .types import SFM_PAIR_REG_DTYPE, SFM_SUMMARY_DTYPE, SFM_VIEW_DTYPE
        own = self._own_inputs()
        kp = np.ascontiguousarray(keypoints, dtype=KEYPOINT_DTYPE)
        m, mk = np.ascontiguousarray(matches, dtype=DMATCH_DTYPE), np.ascontiguousarray(mask, dtype=np.uint8)
        views = np.ascontiguousarray(registration["views"], dtype=SFM_VIEW_DTYPE)
        reg = np.ascontiguousarray(registration["registration"], dtype=SFM_PAIR_REG_DTYPE)
        track = np.ascontiguousarray(registration["track"], dtype=np.int32)
        cloud = np.ascontiguousarray(registration["cloud"], dtype=np.float64).reshape(-1, 3)
        ids = np.ascontiguousarray(registration["cloud_id"], dtype=np.int32)
        summary = np.ascontiguousarray(registration["summary"], dtype=SFM_SUMMARY_DTYPE)
        if (len(kp) < self.total_kp or min(len(m), len(mk), len(track)) < self.total_m or len(views) != self.n_frames or len(reg) != self.n_pairs
                or len(cloud) != len(ids) or len(ids) > self.cloud_cap or len(ids) < min(int(summary["n_tracks"][0]), self.cloud_cap)):
            raise ValueError("keypoints cover every frame; matches, mask and track every pair's match range; one record per pair and per "
                             "frame; the cloud holds its first min(n_tracks, cloud_cap) entries")

        def put(t, a, as_bytes=False):
            a = np.ascontiguousarray(a).reshape(-1)
            flat = torch.from_numpy(a.view(np.uint8) if as_bytes else a)
            if len(flat):
                t[:len(flat)].copy_(flat)
        put(own["kp"], kp[:self.total_kp], 1)
        put(own["matches"], m[:self.total_m], 1)
        put(own["mask"], mk[:self.total_m])
        put(own["views"], views, 1)
        put(own["reg"], reg, 1)
        put(own["track"], track[:self.total_m])
        put(own["cloud"], cloud)
        put(own["cloud_id"], ids)
        put(own["summary"], summary, 1)

    def run(self, after=None, d_kp=None, d_matches=None, d_mask=None):
        """gms_sfm_ba_device, stream-ordered on the context's stream; no allocation, no synchronisation, no readback. after: the
        SfmRegister whose outputs to refine, with the keypoints, survivors and mask on the device; none of them: the object's own."""
        given = (after, d_kp, d_matches, d_mask)
        if all(t is None for t in given):
            o = self._own_inputs()
            ptrs = [o[k].data_ptr() for k in ("kp", "matches", "mask", "views", "reg", "track")] + [o["cloud"].data_ptr(), o["cloud_id"].data_ptr(),
                                                                                               o["summary"].data_ptr()]
        elif any(t is None for t in given):
            raise ValueError("run: a SfmRegister and the three input tensors, or none (the object's own)")
        else:
            if after.cloud_cap != self.cloud_cap or after.n_pairs != self.n_pairs or after.total_kp != self.total_kp:
                raise ValueError("run: the SfmRegister has other sizes")
            ptrs = [d_kp.data_ptr(), d_matches.data_ptr(), d_mask.data_ptr(), after.d_views.data_ptr(), after.d_reg.data_ptr(),
                    after.d_track.data_ptr(), after.d_cloud.data_ptr(), after.d_cloud_id.data_ptr(), after.d_summary.data_ptr()]
        kp, matches, mask, views, reg, track, cloud, cloud_id, summary = ptrs
        self.ctx.sfm_ba_device(self.camera, self.params, kp, self.d_frame_off.data_ptr(), self.n_frames, self.total_kp, self.d_pairs.data_ptr(),
                               self.n_pairs, self.total_m, matches, mask, views, reg, track, self.cloud_cap, cloud, cloud_id, summary,
                               self.d_ws.data_ptr(), self.ws_bytes, self.d_views_out.data_ptr(), self.d_cloud_out.data_ptr(),
                               self.d_status.data_ptr(), self.d_summary.data_ptr())

    def results(self, n_tracks=None):
        """Waits for the context's stream -> dict(views_ba, cloud_ba, track_status, ba_summary) on the host; the cloud arrays cut to
        n_tracks entries when given."""
        from .types import SFM_BA_SUMMARY_DTYPE, SFM_VIEW_DTYPE
        self.ctx.synchronize()
        n = self.cloud_cap if n_tracks is None else min(int(n_tracks), self.cloud_cap)
        return dict(views_ba=self.d_views_out.cpu().numpy().view(SFM_VIEW_DTYPE).copy(), cloud_ba=self.d_cloud_out.cpu().numpy().reshape(-1, 3)[:n].copy(),
                    track_status=self.d_status.cpu().numpy()[:n].copy(), ba_summary=self.d_summary.cpu().numpy().view(SFM_BA_SUMMARY_DTYPE).copy())


def _pose_records(pose_records, views, n):
    """DensePairs' pose_records= and views= -> (d_tv, d_reg, d_pairs, n_frames), checked against n pairs."""
    from .types import SFM_PAIR_REG_DTYPE, SFM_VIEW_DTYPE, TWO_VIEW_DTYPE
    rec = (pose_records.d_tv, pose_records.d_reg, pose_records.d_pairs) if isinstance(pose_records, SfmPairPoses) else tuple(pose_records)
    if len(rec) != 3:
        raise ValueError("pose_records: a SfmPairPoses, or its (d_tv, d_reg, d_pairs)")
    d_tv, d_reg, d_pairs = rec
    for t, size, name in ((d_tv, TWO_VIEW_DTYPE.itemsize, "d_tv"), (d_reg, SFM_PAIR_REG_DTYPE.itemsize, "d_reg"), (d_pairs, PAIR_DTYPE.itemsize, "d_pairs")):
        if t.dtype != torch.uint8 or not t.is_contiguous() or t.numel() != int(n) * size:
            raise ValueError(f"pose_records: {name} holds {int(n)} records of {size} bytes as a contiguous uint8 tensor")
    if views.dtype != torch.uint8 or not views.is_contiguous() or views.numel() == 0 or views.numel() % SFM_VIEW_DTYPE.itemsize:
        raise ValueError(f"views: SFM_VIEW_DTYPE records ({SFM_VIEW_DTYPE.itemsize} bytes each) as a contiguous uint8 device tensor")
    return d_tv, d_reg, d_pairs, views.numel() // SFM_VIEW_DTYPE.itemsize


class SfmPairPoses:
    """Device buffers of gms_sfm_pair_poses_device over a fixed list of frame pairs: the pair table d_pairs
    (PAIR_DTYPE; m and match_off 0) and the records d_tv (TWO_VIEW_DTYPE) and d_reg (SFM_PAIR_REG_DTYPE) of every pair, sized once,
    so that run() can be repeated or captured into a graph; it is one kernel on the context's stream. frame_pairs: (frame_a, frame_b)
    rows -- any two frames of the view array, matched sparsely or not; a pair the views cannot pose (an index out of range, a == b,
    a frame that is not registered, coincident centres, a value that is not finite) gets GMS_ERR_NO_MODEL records. The views are a
    device tensor of n_frames SFM_VIEW_DTYPE records handed to run() (SfmRegister.d_views, SfmBundle.d_views_out), or the object's own,
    which set_views() fills from the host."""

    def __init__(self, ctx, n_frames, frame_pairs, device=None):
        from .types import SFM_PAIR_REG_DTYPE, SFM_VIEW_DTYPE, TWO_VIEW_DTYPE
        self.ctx, self.n_frames = ctx, int(n_frames)
        fp = np.asarray(frame_pairs, dtype=np.int64).reshape(-1, 2)
        if self.n_frames < 1 or (np.abs(fp) > 2 ** 31 - 1).any():
            raise ValueError("SfmPairPoses: at least one frame; frame indices are 32-bit")
        self.frame_pairs, self.n_pairs = fp, len(fp)
        self.recs = np.zeros(self.n_pairs, PAIR_DTYPE)
        self.recs["frame_a"], self.recs["frame_b"] = fp[:, 0], fp[:, 1]
        dev = _device(ctx, device)
        self.device = dev
        n = max(self.n_pairs, 1)
        self.d_pairs = _to_dev(self.recs, dev) if self.n_pairs else torch.zeros(PAIR_DTYPE.itemsize, dtype=torch.uint8, device=dev)
        self.d_tv = torch.zeros(n * TWO_VIEW_DTYPE.itemsize, dtype=torch.uint8, device=dev)
        self.d_reg = torch.zeros(n * SFM_PAIR_REG_DTYPE.itemsize, dtype=torch.uint8, device=dev)
        self._view_bytes = SFM_VIEW_DTYPE.itemsize
        self.d_views = None
        if self.n_pairs == 0:   # (DensePairs takes the tensors by their size)
            self.d_pairs, self.d_tv, self.d_reg = self.d_pairs[:0], self.d_tv[:0], self.d_reg[:0]
        torch.cuda.synchronize(dev)

    def set_views(self, views):
        """n_frames SFM_VIEW_DTYPE records on the host -> the object's own view tensor (the same tensor every time)."""
        from .types import SFM_VIEW_DTYPE
        rec = np.ascontiguousarray(views, dtype=SFM_VIEW_DTYPE).reshape(-1)
        if len(rec) != self.n_frames:
            raise ValueError("set_views: one record per frame")
        if self.d_views is None:
            self.d_views = torch.zeros(self.n_frames * self._view_bytes, dtype=torch.uint8, device=self.device)
        self.d_views.copy_(torch.from_numpy(rec.view(np.uint8).reshape(-1)))
        return self.d_views

    def run(self, d_views=None):
        """gms_sfm_pair_poses_device, stream-ordered on the context's stream; no allocation, no synchronisation, no readback."""
        d_views = self.d_views if d_views is None else d_views
        if d_views is None:
            raise ValueError("run: a device view tensor, or set_views() first")
        if d_views.dtype != torch.uint8 or not d_views.is_contiguous() or d_views.numel() != self.n_frames * self._view_bytes:
            raise ValueError(f"views: {self.n_frames} SFM_VIEW_DTYPE records as a contiguous uint8 device tensor")
        self.ctx.sfm_pair_poses_device(d_views.data_ptr(), self.n_frames, self.d_pairs.data_ptr(), self.n_pairs, self.d_tv.data_ptr(),
                                       self.d_reg.data_ptr())
        return self.d_tv, self.d_reg

    def results(self):
        """Waits for the context's stream -> (TWO_VIEW_DTYPE [n_pairs], SFM_PAIR_REG_DTYPE [n_pairs]) on the host."""
        from .types import SFM_PAIR_REG_DTYPE, TWO_VIEW_DTYPE
        self.ctx.synchronize()
        return (self.d_tv.cpu().numpy().view(TWO_VIEW_DTYPE)[:self.n_pairs].copy(), self.d_reg.cpu().numpy().view(SFM_PAIR_REG_DTYPE)[:self.n_pairs].copy())


def pair_poses(ctx, views, pairs, device=None):
    """The convenience call: views (SFM_VIEW_DTYPE records on the host, or a device tensor of their bytes) and (frame_a, frame_b)
    rows -> the SfmPairPoses after one run (its d_tv, d_reg and d_pairs stay on the device; results() brings the records back)."""
    from .types import SFM_VIEW_DTYPE
    on_dev = torch.is_tensor(views)
    n_frames = views.numel() // SFM_VIEW_DTYPE.itemsize if on_dev else len(np.asarray(views).reshape(-1))
    job = SfmPairPoses(ctx, n_frames, pairs, views.device if on_dev and device is None else device)
    if not on_dev:
        job.set_views(views)
    torch.cuda.synchronize(job.device)
    job.run(views if on_dev else None)
    return job


def bundle_adjust(ctx, keypoints, frame_off, pairs, matches, mask, registration, camera, dist=None, device=None, **ba):
    """The convenience call: host arrays (the keypoints, the two-view stage's pairs, survivors and mask, and a registration's dict) ->
    SfmBundle.results() after one gms_sfm_ba_device run, cut to the cloud's entries."""
    job = SfmBundle(ctx, frame_off, pairs, len(registration["cloud_id"]), camera, dist, device, **ba)
    job.load(keypoints, matches, mask, registration)
    torch.cuda.synchronize(job.device)
    job.run()
    return job.results()


def register_pairs(ctx, frame_off, pairs, matches, mask, points3d, two_view, root=0, min_links=8, cloud_cap=None, device=None, keep=None):
    """The convenience call: host arrays of many pairs' two-view results (run_dataset's pairs, out, mask, points3d, two_view and the
    frames' offsets) -> SfmRegister.results() after one gms_sfm_register_device run. keep: a host keep plane (unique_matches') -> one
    gms_sfm_register_keep_device run on it."""
    job = SfmRegister(ctx, frame_off, pairs, root, min_links, cloud_cap, device, keep=None if keep is None else True)
    job.load(matches, mask, points3d, two_view, keep)
    torch.cuda.synchronize(job.device)
    job.run()
    return job.results()
