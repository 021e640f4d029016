"""Directions, map sizes and a rotation shared by the environment-map tests (plain numpy)."""
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
