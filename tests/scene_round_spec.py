"""numpy / plain-Python statement of the self-training round on whole scenes (include/stcd_hip.h: stcd_scene_cell_agree,
stcd_mask_close; stcd_amd/selftrain.py: scene_round).  Loops and bincount, one cell and one pixel at a time: this is the
specification the kernels and the driver are held to.  It says what train_stcd.py:118-125 computes per pre-cut crop
and what cv2.morphologyEx(img, cv2.MORPH_CLOSE, np.ones((5, 5))) of :186-188 computes with OpenCV's default border.  Not collected
by pytest."""
import numpy as np


def grid(height, width, cell):
    """(cells_y, cells_x) = ceil(height / cell), ceil(width / cell)."""
    return -(-height // cell), -(-width // cell)


def cell_agree(masks, cell, label=None):
    """masks: K uint8 [H,W] arrays (non-zero is change, the last plays the label) -> (agree int64 [cells,K-1,4] or None for K == 1,
    cm int64 [cells,4] or None); agree[c, i, 2 * last + pred_i], cm[c, 2 * label + pred_last] (label >= 1 is change, 255 is ignored),
    c = cy * cells_x + cx; edge cells are cut off at the border."""
    masks = [np.asarray(m) for m in masks]
    H, W = masks[0].shape
    K = len(masks)
    cells_y, cells_x = grid(H, W, cell)
    agree = np.zeros((cells_y * cells_x, K - 1, 4), np.int64) if K > 1 else None
    cm = np.zeros((cells_y * cells_x, 4), np.int64) if label is not None else None
    for cy in range(cells_y):
        for cx in range(cells_x):
            c = cy * cells_x + cx
            win = (slice(cy * cell, min(H, (cy + 1) * cell)), slice(cx * cell, min(W, (cx + 1) * cell)))
            last = (masks[-1][win] != 0).astype(np.int64).ravel()
            for i in range(K - 1):
                pred = (masks[i][win] != 0).astype(np.int64).ravel()
                agree[c, i] = np.bincount(2 * last + pred, minlength=4)
            if label is not None:
                lab = np.asarray(label)[win].ravel()
                ok = lab != 255
                cm[c] = np.bincount(2 * (lab[ok] >= 1).astype(np.int64) + last[ok], minlength=4)
    return agree, cm


def cell_pixels(height, width, cell):
    """int64 [cells]: the real pixel count of every cell, row-major."""
    cells_y, cells_x = grid(height, width, cell)
    return np.array([(min(height, (cy + 1) * cell) - cy * cell) * (min(width, (cx + 1) * cell) - cx * cell)
                     for cy in range(cells_y) for cx in range(cells_x)], np.int64)


def full_cells(height, width, cell):
    """bool [cells_y, cells_x]: the cell is a whole cell x cell square."""
    cells_y, cells_x = grid(height, width, cell)
    return np.array([[(cy + 1) * cell <= height and (cx + 1) * cell <= width for cx in range(cells_x)] for cy in range(cells_y)], bool).reshape(cells_y, cells_x)


def cell_names(height, width, cell, stem="scene"):
    cells_y, cells_x = grid(height, width, cell)
    return [f"{stem}_{cy:04d}_{cx:04d}.png" for cy in range(cells_y) for cx in range(cells_x)]


def dilate(m, radius):
    """bool [H,W]: a pixel is set if any pixel of its (2 r + 1)^2 window INSIDE the scene is set."""
    H, W = m.shape
    out = np.zeros((H, W), bool)
    for y in range(H):
        for x in range(W):
            hit = False
            for yy in range(max(0, y - radius), min(H, y + radius + 1)):
                for xx in range(max(0, x - radius), min(W, x + radius + 1)):
                    hit = hit or bool(m[yy, xx])
            out[y, x] = hit
    return out


def erode(m, radius):
    """bool [H,W]: a pixel stays set if every pixel of its window INSIDE the scene is set (positions outside never contribute)."""
    H, W = m.shape
    out = np.zeros((H, W), bool)
    for y in range(H):
        for x in range(W):
            keep = True
            for yy in range(max(0, y - radius), min(H, y + radius + 1)):
                for xx in range(max(0, x - radius), min(W, x + radius + 1)):
                    keep = keep and bool(m[yy, xx])
            out[y, x] = keep
    return out


def close(mask, radius, mask_value=1):
    """uint8 [H,W] (non-zero is set) -> uint8 [H,W], mask_value where set: dilation, then erosion, with the square of edge 2 r + 1."""
    m = np.asarray(mask) != 0
    return (erode(dilate(m, radius), radius) * mask_value).astype(np.uint8)


def close_fast(mask, radius, mask_value=1):
    """The same closing by 2 (2 r + 1) shifted ORs / ANDs of padded arrays: for the larger shapes of the GPU tests.  The CPU tests
    hold it to `close`."""
    m = np.asarray(mask) != 0
    H, W = m.shape
    k = 2 * radius + 1

    def sweep(a, fill, op):
        p = np.pad(a, radius, constant_values=fill)
        acc = p[0:H]
        for d in range(1, k):
            acc = op(acc, p[d:d + H])
        out = acc[:, 0:W]
        for d in range(1, k):
            out = op(out, acc[:, d:d + W])
        return out

    return (sweep(sweep(m, False, np.logical_or), True, np.logical_and) * mask_value).astype(np.uint8)
