"""numpy restatement of the three whole-scene kernels (include/stcd_hip.h: stcd_scene_gather / _stitch / _finalize), float64.

The reference has no scene tiler or overlap blend (it crops offline, /root/reference/split.py:17-46, and scores crops one by
one), so this module states the library's own specification; the GPU tests hold the kernels to it and the CPU tests hold the
closed forms used here to a brute-force scan.  Not an oracle of the reference: it lives beside the tests."""
import numpy as np


def tiles_along(length, tile, stride):
    """max(0, ceil((length - tile) / stride)) + 1"""
    return max(0, -(-(length - tile) // stride)) + 1


def reflect(i, length):
    """Mirror reflection without repeating the edge sample (numpy.pad mode='reflect'), any integer i (array or scalar)."""
    i = np.asarray(i, dtype=np.int64)
    if length == 1:
        return np.zeros_like(i)
    m = 2 * (length - 1)
    i = ((i % m) + m) % m
    return np.where(i >= length, m - i, i)


def covering(p, tile, stride, tiles):
    """Closed form: the tiles k along one axis with k * stride <= p < k * stride + tile are lo..hi (inclusive)."""
    p = np.asarray(p, dtype=np.int64)
    lo = np.where(p < tile, 0, (p - tile) // stride + 1)
    hi = np.minimum(p // stride, tiles - 1)
    return lo, hi


def covering_brute(p, tile, stride, tiles):
    return [k for k in range(tiles) if k * stride <= p < k * stride + tile]


def gather(scene, tile, stride, tiles_x, first_tile, n_tiles, mean, std):
    """uint8 [H,W,3] -> float64 [n_tiles,3,T,T]: (u / 255 - mean) / std of the reflected scene."""
    H, W, _ = scene.shape
    out = np.empty((n_tiles, 3, tile, tile), np.float64)
    t = np.arange(tile)
    mean, std = np.asarray(mean, np.float64), np.asarray(std, np.float64)
    for n in range(n_tiles):
        ky, kx = divmod(first_tile + n, tiles_x)
        ys, xs = reflect(ky * stride + t, H), reflect(kx * stride + t, W)
        crop = scene[ys][:, xs].astype(np.float64)                      # [T,T,3]
        out[n] = ((crop / 255.0 - mean) / std).transpose(2, 0, 1)
    return out


def stitch(logits, height, width, tile, stride, tiles_x, tiles_y, first_tile, window, acc, wsum):
    """logits [n,classes,T,T] of tiles first_tile.. are added into float64 acc [classes,H,W] / wsum [H,W] in place, ascending tile
    index; the pixels a tile reaches are decided by the closed form `covering`, as in the kernel."""
    n_tiles = logits.shape[0]
    win = np.ones(tile, np.float64) if window is None else np.asarray(window).astype(np.float64)
    ylo, yhi = covering(np.arange(height), tile, stride, tiles_y)
    xlo, xhi = covering(np.arange(width), tile, stride, tiles_x)
    for n in range(n_tiles):
        ky, kx = divmod(first_tile + n, tiles_x)
        ys = np.nonzero((ylo <= ky) & (ky <= yhi))[0]
        xs = np.nonzero((xlo <= kx) & (kx <= xhi))[0]
        if ys.size == 0 or xs.size == 0:
            continue
        ty, tx = ys - ky * stride, xs - kx * stride
        w = win[ty][:, None] * win[tx][None, :]
        acc[:, ys[:, None], xs[None, :]] += w[None] * logits[n].astype(np.float64)[:, ty[:, None], tx[None, :]]
        wsum[ys[:, None], xs[None, :]] += w
    return acc, wsum


def finalize(acc, wsum, threshold=0.0, label=None):
    """-> (mask uint8 [H,W], prob float64 [H,W], cm int64 [4] or None)."""
    acc, wsum = np.asarray(acc, np.float64), np.asarray(wsum, np.float64)
    if acc.shape[0] == 2:
        mask = acc[1] > acc[0]                                          # a tie is class 0
        d = (acc[1] - acc[0]) / wsum
    else:
        mask = acc[0] > threshold * wsum                                # on the threshold is class 0
        d = acc[0] / wsum
    with np.errstate(over="ignore"):
        prob = 1.0 / (1.0 + np.exp(-d))                                 # softmax class 1 of two == sigmoid of the difference
    cm = None
    if label is not None:
        ok = label != 255
        cm = np.bincount(2 * (label[ok] >= 1).astype(np.int64) + mask[ok].astype(np.int64), minlength=4).astype(np.int64)
    return mask.astype(np.uint8), prob, cm
