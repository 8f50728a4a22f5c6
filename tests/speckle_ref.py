"""The speckle filter (cv::filterSpeckles for CV_16S) stated twice in numpy, independently of each other and of
sfm-gms_amd/csrc/speckle_core.h. Written from the published algorithm: parity with an OpenCV binary is unpinned.

Two pixels are linked when they are 4-neighbours, neither equals new_val, and |a - b| <= max_diff with the difference taken beyond 16
bits. Components are the transitive closure. Every pixel that is not new_val and whose component has at most max_speckle_size pixels
becomes new_val. Both functions return (filtered copy, pixels changed)."""
import numpy as np


def check_args(disp16, new_val, max_speckle_size, max_diff):
    d = np.asarray(disp16)
    if d.dtype != np.int16 or d.ndim != 2 or d.size == 0 or max(d.shape) > 8192:
        raise ValueError("disp16: int16 [H, W], sides 1..8192")
    if not -32768 <= int(new_val) <= 32767 or int(max_speckle_size) < 0 or int(max_diff) < 0:
        raise ValueError("new_val within int16, max_speckle_size >= 0, max_diff >= 0")
    return d


def literal(disp16, new_val, max_speckle_size, max_diff):
    """The raster scan with an explicit flood-fill stack, as cv::filterSpeckles does it: a label plane, a flag per label that says
    whether the region was small, and the fill that counts the region before it decides."""
    img = check_args(disp16, new_val, max_speckle_size, max_diff).copy()
    h, w = img.shape
    new_val, max_speckle_size, max_diff = int(new_val), int(max_speckle_size), int(max_diff)
    labels = np.zeros((h, w), np.int32)
    small = [False]                      # per label (0: none yet)
    rows = img.tolist()                  # Python ints: differences cannot wrap
    lab = labels.tolist()
    removed = 0
    for i in range(h):
        for j in range(w):
            if rows[i][j] == new_val:
                continue
            if lab[i][j]:
                if small[lab[i][j]]:
                    rows[i][j] = new_val
                    removed += 1
                continue
            cur = len(small)
            lab[i][j] = cur
            stack, count = [(i, j)], 0
            while stack:
                y, x = stack.pop()
                count += 1
                v = rows[y][x]
                for yn, xn in ((y, x + 1), (y, x - 1), (y + 1, x), (y - 1, x)):
                    if 0 <= yn < h and 0 <= xn < w and not lab[yn][xn] and rows[yn][xn] != new_val and abs(v - rows[yn][xn]) <= max_diff:
                        lab[yn][xn] = cur
                        stack.append((yn, xn))
            small.append(count <= max_speckle_size)
            if small[cur]:
                rows[i][j] = new_val
                removed += 1
    return np.array(rows, dtype=np.int16).reshape(h, w), removed


def component_labels(disp16, new_val, max_diff):
    """int64 [H, W]: the lowest raster index of the pixel's component, -1 where the pixel is new_val. Minimum-label propagation over
    the links to a fixed point, with pointer jumping between the sweeps."""
    d = np.asarray(disp16).astype(np.int64)
    h, w = d.shape
    live = d != int(new_val)
    right = live[:, :-1] & live[:, 1:] & (np.abs(d[:, :-1] - d[:, 1:]) <= int(max_diff))    # (y, x) -- (y, x + 1)
    down = live[:-1, :] & live[1:, :] & (np.abs(d[:-1, :] - d[1:, :]) <= int(max_diff))     # (y, x) -- (y + 1, x)
    lab = np.arange(h * w, dtype=np.int64).reshape(h, w)
    while True:
        new = lab.copy()
        np.minimum(new[:, :-1], np.where(right, lab[:, 1:], new[:, :-1]), out=new[:, :-1])
        np.minimum(new[:, 1:], np.where(right, lab[:, :-1], new[:, 1:]), out=new[:, 1:])
        np.minimum(new[:-1, :], np.where(down, lab[1:, :], new[:-1, :]), out=new[:-1, :])
        np.minimum(new[1:, :], np.where(down, lab[:-1, :], new[1:, :]), out=new[1:, :])
        flat = new.reshape(-1)
        while True:                      # pointer jumping: a label is a pixel of the same component with a label no higher
            hop = flat[flat]
            if np.array_equal(hop, flat):
                break
            flat = hop
        new = flat.reshape(h, w)
        if np.array_equal(new, lab):
            break
        lab = new
    return np.where(live, lab, -1)


def components(disp16, new_val, max_speckle_size, max_diff):
    """Labels by propagation, sizes by bincount."""
    d = check_args(disp16, new_val, max_speckle_size, max_diff)
    lab = component_labels(d, new_val, max_diff)
    live = lab >= 0
    sizes = np.bincount(lab[live], minlength=d.size)
    kill = live & (sizes[np.where(live, lab, 0)] <= int(max_speckle_size))
    out = d.copy()
    out[kill] = np.int16(new_val)
    return out, int(kill.sum())
