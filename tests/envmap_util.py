"""Directions, map sizes, a rotation, a test map and the records' per-pixel sums shared by the
environment-map tests (plain numpy)."""
import itertools

import numpy as np

SIZES = [(2, 2), (7, 5), (64, 32)]  # (W, H)
SPECIAL = [0.0, -0.0, 1.0, -1.0, float("nan"), float("inf"), float("-inf"), 1e-30, -1e-30, 0.7071, -0.7071,
           1.0000001]
ROT = np.array([[0.36, 0.48, -0.8], [-0.8, 0.6, 0.0], [0.48, 0.64, 0.6]], np.float32)  # a rotation, rounded


def special_dirs():
    """Every triple of the special values (the issue's list; +1.0000001 overshoots the acos clamp)."""
    return np.array(list(itertools.product(SPECIAL, repeat=3)), np.float32)


def random_dirs(n, seed=5):
    rng = np.random.default_rng(seed)
    d = rng.standard_normal((n, 3))
    return (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)


def env_image(W, H, seed=0, channels=3):
    """A positive map with structure in both directions and a bright patch (a 'sun')."""
    rng = np.random.default_rng(100 + seed + W)
    yy, xx = np.mgrid[0:H, 0:W]
    img = np.zeros((H, W, channels), np.float32)
    for c in range(3):
        img[..., c] = (0.2 + 0.8 * rng.random((H, W)) + np.sin(2 * np.pi * xx / W + c) ** 2 + yy / H).astype(np.float32)
    img[H // 3, W // 2, :3] = (40.0, 30.0, 20.0)
    if channels == 4:
        img[..., 3] = -7.0  # ignored: never read into the stored texels
    return img


def record_sums(rec, tile, iters, field="C", square=False):
    """fp64 per-pixel sums of the records' contributions (square: of their fp32 squares)."""
    px = tile[0] * tile[1]
    v = rec[field].astype(np.float32)
    if square:
        v = (v * v).astype(np.float32)
    return v.astype(np.float64).reshape(iters, px, 3).sum(axis=0).reshape(tile[1], tile[0], 3)
