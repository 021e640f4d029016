"""The BSDF / box / camera parameter cases shared by tests/test_params_cpu.py (oracle pins, sharpness
and coverage on the CPU) and tests/test_gpu_params.py (GPU == oracle).  Plain numpy, no library call.

Medium: blob16, a 16^3 density blob with a non-uniform albedo, scale 40, majorant 1.
Launch: 32x32 pixels = the full resolution, 4 samples (4096 paths), seed 7; one extra launch renders
tile 32x24 at offset (32, 24) of a 64x48 image.
Cameras: 12-float inv_view arrays built by hand.  Columns 0..2 of the 3x4 row-major matrix are the
camera's right, up and forward axes in world space, column 3 the eye; camera_ray computes
d = R normalize(rx, ry, 1).  A pencil camera has raster_to_view (0, 0): every path gets the ray
(eye, dir) and only the RNG differs.  (The zero components of a pencil's direction are sums of signed
zeros: all +0 for pencil_in, of either sign, depending on the pixel's side of the image centre, for
pencil_negzero.)"""
from collections import namedtuple

import numpy as np

SCALE = 40.0
MAX_DENSITY = 1.0
W = H = 32
SAMPLES = 4
SEED = 7
DEFAULT_ETA = float(np.float32(np.float32(1.05) / np.float32(1.01)))
DEFAULTS = dict(g=0.0, roughness=(0.1, 0.1), eta=DEFAULT_ETA, box_min=(-0.5,) * 3, box_max=(0.5,) * 3)

# inv_view (12 floats), raster_to_view (2 floats)
Camera = namedtuple("Camera", "inv_view r2v")
# params: the fields that differ from DEFAULTS; camera: a key of camera(); w2a: CVR_OPT_WORLD_TO_AABB;
# full / tile / offset: the launch geometry
Case = namedtuple("Case", "params camera w2a full tile offset")


def blob16():
    """(density (16, 16, 16) f32, albedo (16, 16, 16, 4) f32)."""
    z, y, x = np.meshgrid(*(np.linspace(-1, 1, 16),) * 3, indexing="ij")
    rs = np.random.RandomState(1)
    density = np.clip(1.2 - np.sqrt(x * x + y * y + z * z), 0, 1) * rs.uniform(0.3, 1, (16, 16, 16))
    albedo = np.ones((16, 16, 16, 4), np.float32)
    albedo[..., :3] = rs.uniform(0.5, 1.0, (16, 16, 16, 3))
    return density.astype(np.float32), albedo


def _unit(v):
    v = np.asarray(v, np.float64)
    return v / np.linalg.norm(v)


def inv_view(R, eye):
    M = np.zeros((3, 4), np.float32)
    M[:, :3] = R
    M[:, 3] = eye
    return M.ravel()


def look_at_R(eye, at, up=(0, 1, 0)):
    """Columns right, up, forward, with the handedness of the default camera (right (1, 0, 0),
    up (0, -1, 0), forward (0, 0, -1))."""
    f = _unit(np.subtract(at, eye, dtype=np.float64))
    r = _unit(np.cross(f, np.asarray(up, np.float64)))
    u = np.cross(f, r)
    return np.stack([r, u, f], axis=1).astype(np.float32)


def look_at(eye, at, up=(0, 1, 0), fov=20.0, full=(W, H)):
    t = np.tan(np.radians(fov) / 2)
    return Camera(inv_view(look_at_R(eye, at, up), eye), np.array([t, t * full[1] / full[0]], np.float32))


def pencil(eye, direction):
    d = np.asarray(direction, np.float32)
    up = (0, 1, 0) if abs(d[1]) < 0.9 else (1, 0, 0)
    R = look_at_R((0, 0, 0), d.astype(np.float64), up)
    R[:, 2] = d  # literally, signed zeros included
    return Camera(inv_view(R, eye), np.zeros(2, np.float32))


CAMERAS = {
    "front": lambda full: look_at((0, 0, 4), (0, 0, 0), fov=20.0, full=full),
    "oblique": lambda full: look_at((2.1, 1.3, -1.7), (0.1, 0, 0), (0.2, 1, 0.1), fov=40.0, full=full),
    # (eye (0.1, -0.05, 0.2) towards (0.5, 0.4, -0.3) lies so deep in the blob that 8 % of the paths
    # reach a boundary: eta := 1/eta changed 0.5 % of them, below the 1 % of tests/test_params_cpu.py)
    "inside": lambda full: look_at((0.4, -0.3, 0.35), (0.0, 0.4, -0.5), fov=90.0, full=full),
    "pencil_in": lambda full: pencil((0.25, -0.125, 4), (0.0, 0.0, -1.0)),
    "pencil_negzero": lambda full: pencil((0.25, -0.125, 4), (-0.0, -0.0, -1.0)),
    "pencil_face": lambda full: pencil((0.5, 0.1, 4), (0.0, 0.0, -1.0)),      # eye on the x = 0.5 plane
    "pencil_edge": lambda full: pencil((0.5, -0.5, 4), (0.0, 0.0, -1.0)),
    "pencil_out": lambda full: pencil((0.75, 0, 4), (0.0, 0.0, -1.0)),        # a miss
    # starts inside, along x ((0, 0.1, 0.2) for the same reason as above: 0.3 %)
    "pencil_x_inside": lambda full: pencil((0.4, 0.1, 0.2), (1.0, 0.0, 0.0)),
    "pencil_in_plane": lambda full: pencil((-3, 0.5, 0.1), (1.0, 0.0, 0.0)),  # travels in the y = 0.5 plane
}
PENCILS = [k for k in CAMERAS if k.startswith("pencil_")]
ALL_MISS = ["pencil_face", "pencil_edge", "pencil_out", "pencil_in_plane"]


def camera(name, full=(W, H)):
    return CAMERAS[name](full)


def _case(params=None, cam="front", w2a=0, full=(W, H), tile=(W, H), offset=(0, 0)):
    return Case(dict(params or {}), cam, w2a, full, tile, offset)


_BOX_ALL = dict(box_min=(-0.3, -0.2, -0.4), box_max=(0.5, 0.4, 0.8), g=0.5, roughness=(0.15, 0.3))
CASES = {
    "default": _case(),
    "g_pos": _case(dict(g=0.6)),
    "g_neg": _case(dict(g=-0.4), "oblique"),
    "aniso_a": _case(dict(roughness=(0.05, 0.4)), "oblique"),
    "aniso_b": _case(dict(roughness=(0.5, 0.02))),
    "eta_one": _case(dict(eta=1.0), "oblique"),
    "eta_lt1": _case(dict(eta=float(np.float32(1 / 1.5))), "oblique"),
    "eta_big": _case(dict(eta=1.5, roughness=(0.3, 0.3))),
    "inside": _case(None, "inside"),
    "inside_all": _case(dict(g=0.3, roughness=(0.2, 0.35), eta=1.33), "inside"),
    "box_all": _case(_BOX_ALL, "oblique", 0),
    "box_all_w2a": _case(_BOX_ALL, "oblique", 1),
    "oblique_offset": _case(None, "oblique", 0, (64, 48), (32, 24), (32, 24)),
}
CASES.update({k: _case(None, k) for k in PENCILS})
COMBINED = ["inside_all", "box_all", "box_all_w2a"]
# the roughness pairs of the cases (the pins also take both swaps)
ROUGHNESS = sorted({tuple(c.params["roughness"]) for c in CASES.values() if "roughness" in c.params}
                   | {DEFAULTS["roughness"]})


def medium_params(case, **override):
    p = dict(DEFAULTS)
    p.update(case.params)
    p.update(override)
    return p


def at_tile(case, tile):
    """The case's view rendered as an image of tile[0] x tile[1] pixels of its own (full = tile, no
    offset): the same camera and parameters at another pixel count.  (A camera's raster_to_view depends
    on the aspect alone, so a square case keeps its view at any square size.)"""
    return case._replace(full=tuple(tile), tile=tuple(tile), offset=(0, 0))


def n_paths(case, samples=SAMPLES):
    return case.tile[0] * case.tile[1] * samples


def make_oracle(oracle_mod, case, density=None, albedo=None, max_density=MAX_DENSITY, **override):
    """The oracle over blob16 (or the given arrays) with the case's parameters."""
    if density is None:
        density, albedo = blob16()
    p = medium_params(case, **override)
    return oracle_mod.Oracle(density, albedo, p["box_min"], p["box_max"], SCALE, max_density, p["g"],
                             p["roughness"], p["eta"])


def make_launch(oracle_mod, case, kernel, cam=None, w2a=None):
    cam = camera(case.camera, case.full) if cam is None else cam
    return oracle_mod.Oracle.launch(cam.inv_view, cam.r2v, case.full, case.tile, case.offset, kernel, SEED,
                                    world_to_aabb=case.w2a if w2a is None else w2a)
