"""ctypes binding of libcvr.so (include/cvr.h).

This is the only way Python reaches the renderer: every call goes through the
C ABI that a C/C++/Go/Java host would bind.  There is no
Python or CPU fallback: if libcvr.so is missing or a HIP call fails, the call
raises.
"""
from __future__ import annotations

import ctypes as C
import math
import os
from collections import namedtuple
from typing import Optional, Sequence

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_DEFAULT_LIB = os.path.abspath(os.path.join(_HERE, "libcvr.so"))
# CVR_LIB: an experiment build instead of the in-tree library (e.g. `make variant NAME=u2 ...`'s
# build/variants/u2/libcvr.so); unset, the in-tree libcvr.so
LIB_PATH = os.environ.get("CVR_LIB") or _DEFAULT_LIB

CVR_OK = 0
ERRORS = {-1: "CVR_ERR_INVALID", -2: "CVR_ERR_HIP", -3: "CVR_ERR_STATE", -4: "CVR_ERR_IO",
          -5: "CVR_ERR_UNSUPPORTED", -6: "CVR_ERR_NOMEM"}

# Config::Kernel order (Config.h:87-95)
KERNELS = ["naiveSK", "naiveMK", "regenerationSK", "streamingMK", "streamingSK", "sortingSK"]
NAIVE_SK, NAIVE_MK, REGENERATION_SK, STREAMING_MK, STREAMING_SK, SORTING_SK = range(6)
SCENE_TYPES = {"Auto": 0, "MitsubaXml": 1, "Vdb": 2, "Raw": 3, "Mhd": 4, "VdbSparse": 5}

OPT_MAX_SEGMENTS, OPT_CHUNK, OPT_EVENT_THRESHOLD, OPT_GRID, OPT_SCATTER_EPS = 1, 2, 3, 4, 5
OPT_SCHEDULER, OPT_POOL, OPT_TIMING, OPT_CELLS, OPT_WAVES, OPT_ORDER, OPT_QUEUES = 6, 7, 8, 9, 10, 11, 12
OPT_BOUNDS, OPT_TAIL, OPT_BATCH, OPT_RNG_BINDING, OPT_MORTON = 13, 14, 15, 16, 17
OPT_WORLD_TO_AABB, OPT_MK_COMPACTION, OPT_SUBQUEUES, OPT_DRAIN, OPT_INFLIGHT, OPT_FRAME_FLUSH = 18, 19, 20, 22, 23, 24
OPT_UNIFORM_ALBEDO, OPT_WAVE_PAIR, OPT_SAMPLE_ORDER, OPT_EMPTY_MASK, OPT_COUNT_WORDS = 25, 26, 27, 28, 29
OPT_MEDIUM_FORMAT = 30
OPT_MOMENTS = 31  # per-pixel second moments behind the tile (Context.copy_moments)
FORMAT_F32, FORMAT_F16 = 0, 1  # OPT_MEDIUM_FORMAT: storage precision of the voxel values in HBM


class CvrError(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__(f"{ERRORS.get(code, code)}: {msg}")
        self.code = code


class MediumDesc(C.Structure):
    _fields_ = [("res", C.c_uint32 * 3), ("density", C.POINTER(C.c_float)),
                ("albedo", C.POINTER(C.c_float)), ("box_min", C.c_float * 3),
                ("box_max", C.c_float * 3), ("scale", C.c_float), ("max_density", C.c_float),
                ("g", C.c_float), ("roughness", C.c_float * 2), ("eta", C.c_float)]


NO_LEAF = 0xFFFFFFFF


class SparseMediumDesc(C.Structure):
    _fields_ = [("res", C.c_uint32 * 3), ("leaf_dims", C.c_uint32 * 3),
                ("leaf_table", C.POINTER(C.c_uint32)), ("n_leaves", C.c_uint32),
                ("leaf_density", C.POINTER(C.c_float)), ("leaf_albedo", C.POINTER(C.c_float)),
                ("albedo_background", C.c_float * 4), ("box_min", C.c_float * 3),
                ("box_max", C.c_float * 3), ("scale", C.c_float), ("max_density", C.c_float),
                ("g", C.c_float), ("roughness", C.c_float * 2), ("eta", C.c_float)]


class Stats(C.Structure):
    _fields_ = [("paths", C.c_uint64), ("segments", C.c_uint64), ("steps", C.c_uint64),
                ("density", C.c_uint64), ("albedo", C.c_uint64), ("escaped", C.c_uint64),
                ("truncated", C.c_uint64), ("kernel_ms", C.c_double), ("iterations", C.c_uint64),
                ("track_ms", C.c_double), ("events_ms", C.c_double), ("fetches", C.c_uint64),
                ("words", C.c_uint64)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class MediumInfo(C.Structure):
    """cvr_medium_info: format and device bytes of a context's medium."""
    _fields_ = [("format", C.c_int32), ("max_density_eff", C.c_float), ("density_bytes", C.c_uint64),
                ("cells_bytes", C.c_uint64), ("albedo_bytes", C.c_uint64), ("bounds_bytes", C.c_uint64),
                ("total_bytes", C.c_uint64)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class PathRecord(C.Structure):
    _fields_ = [("image_id", C.c_uint32), ("flags", C.c_uint32), ("T", C.c_float * 3),
                ("n_segments", C.c_uint32), ("n_steps", C.c_uint32), ("n_density", C.c_uint32),
                ("n_albedo", C.c_uint32)]


PATH_RECORD_DTYPE = np.dtype([("image_id", "<u4"), ("flags", "<u4"), ("T", "<f4", (3,)),
                              ("n_segments", "<u4"), ("n_steps", "<u4"), ("n_density", "<u4"),
                              ("n_albedo", "<u4")])
assert PATH_RECORD_DTYPE.itemsize == C.sizeof(PathRecord)


class LoadOptions(C.Structure):
    _fields_ = [("flags", C.c_uint32), ("default_albedo", C.c_float * 3)]


LOAD_DEFAULT_ALBEDO = 1


class RenderDesc(C.Structure):
    _fields_ = [("resolution", C.c_uint32 * 2), ("n_tiles", C.c_uint32 * 2), ("iterations", C.c_uint32)]


class AdaptiveDesc(C.Structure):
    """cvr_adaptive_desc: the sampling plan of a noise-targeted render."""
    _fields_ = [("min_iterations", C.c_uint32), ("max_iterations", C.c_uint32), ("pass_iterations", C.c_uint32),
                ("target", C.c_float), ("floor", C.c_float)]

    def __init__(self, min_iterations=8, max_iterations=32, pass_iterations=4, target=0.05, floor=0.01):
        super().__init__(min_iterations, max_iterations, pass_iterations, target, floor)


class AdaptiveResult(C.Structure):
    """cvr_adaptive_result: the session's state after a pass."""
    _fields_ = [("passes", C.c_uint32), ("blocks", C.c_uint32), ("blocks_active", C.c_uint32),
                ("paths", C.c_uint64), ("max_error", C.c_double), ("mean_error", C.c_double),
                ("done", C.c_int32)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class DenoiseDesc(C.Structure):
    """cvr_denoise_desc: the variance-guided a-trous filter's parameters (passes 1..6, pass k with
    step 2^k; sigma: width of the edge-stopping term in standard deviations; floor > 0)."""
    _fields_ = [("passes", C.c_uint32), ("sigma", C.c_float), ("floor", C.c_float), ("flags", C.c_uint32)]

    def __init__(self, passes=5, sigma=4.0, floor=0.01, flags=0):
        super().__init__(passes, sigma, floor, flags)


class FeaturesDesc(C.Structure):
    """cvr_features_desc: the primary-ray feature pass (step in cells of the finest axis, 1/8..8;
    t_stop: the transmittance below which a ray's march ends, 0 = never; max_steps 1..65536)."""
    _fields_ = [("step", C.c_float), ("t_stop", C.c_float), ("max_steps", C.c_uint32), ("flags", C.c_uint32)]

    def __init__(self, step=1.0, t_stop=1.0 / 256.0, max_steps=4096, flags=0):
        super().__init__(step, t_stop, max_steps, flags)


class DenoiseGuidedDesc(C.Structure):
    """cvr_denoise_guided_desc: the denoiser's parameters (base) and the widths of the three feature
    terms (albedo, depth, opacity; <= 0 switches a term off)."""
    _fields_ = [("base", DenoiseDesc), ("sigma_albedo", C.c_float), ("sigma_depth", C.c_float),
                ("sigma_alpha", C.c_float), ("flags", C.c_uint32)]

    def __init__(self, base: Optional[DenoiseDesc] = None, sigma_albedo=0.4, sigma_depth=0.1, sigma_alpha=0.4, flags=0):
        super().__init__(DenoiseDesc() if base is None else base, sigma_albedo, sigma_depth, sigma_alpha, flags)


PREVIEW_UNSHADED, PREVIEW_HEADLIGHT = 1, 2


class PreviewDesc(C.Structure):
    """cvr_preview_desc: the shaded preview pass.  march: the feature pass's descriptor; light: the
    direction towards the light (read only without PREVIEW_HEADLIGHT and PREVIEW_UNSHADED);
    ambient, diffuse, specular: the Blinn-Phong weights, the specular exponent 2^shininess_log2;
    knee: the gradient magnitude, in units of max_density per finest cell, at which a sample is
    half lit; background: the colour behind the medium."""
    _fields_ = [("march", FeaturesDesc), ("light", C.c_float * 3), ("ambient", C.c_float), ("diffuse", C.c_float),
                ("specular", C.c_float), ("shininess_log2", C.c_uint32), ("knee", C.c_float),
                ("background", C.c_float * 3), ("flags", C.c_uint32)]

    def __init__(self, march: Optional[FeaturesDesc] = None, light=None, ambient=0.3, diffuse=0.7, specular=0.2,
                 shininess_log2=4, knee=0.05, background=(0.0, 0.0, 0.0), flags=None):
        """flags None: PREVIEW_HEADLIGHT unless a light is given."""
        if flags is None:
            flags = PREVIEW_HEADLIGHT if light is None else 0
        light = (0.0, 0.0, 0.0) if light is None else light
        super().__init__(FeaturesDesc() if march is None else march, (C.c_float * 3)(*[float(v) for v in light]),
                         ambient, diffuse, specular, shininess_log2, knee,
                         (C.c_float * 3)(*[float(v) for v in background]), flags)


class LightVolumeDesc(C.Structure):
    """cvr_light_volume_desc: the light volume of the shadowed preview.  res: its nodes per axis
    (x, y, z), each 1..1024; light: the direction towards the light, any length; march: the feature
    pass's descriptor for the march from each node towards the light."""
    _fields_ = [("res", C.c_uint32 * 3), ("flags", C.c_uint32), ("light", C.c_float * 3), ("reserved", C.c_float),
                ("march", FeaturesDesc)]

    def __init__(self, res=(1, 1, 1), light=(0.0, 0.0, 1.0), march: Optional[FeaturesDesc] = None, flags=0):
        super().__init__((C.c_uint32 * 3)(*[int(v) for v in res]), flags, (C.c_float * 3)(*[float(v) for v in light]),
                         0.0, FeaturesDesc() if march is None else march)


class LightVolumeInfo(C.Structure):
    """cvr_light_volume_info: the context's light volume (valid 0: none, everything 0)."""
    _fields_ = [("res", C.c_uint32 * 3), ("valid", C.c_uint32), ("light", C.c_float * 3), ("reserved", C.c_float),
                ("bytes", C.c_uint64)]

    def as_dict(self):
        return {"res": tuple(self.res), "valid": bool(self.valid), "light": tuple(self.light), "bytes": self.bytes}


DEVMED_SPARSE, DEVMED_CONST_ALBEDO, DEVMED_MAX_DENSITY = 1, 2, 4
# cvr_debug_copy_medium's arrays (CVR_MEDIUM_*), by index
MEDIUM_ARRAYS = ("density", "albedo", "cells", "bounds", "leaf_table", "leaf_density", "leaf_albedo", "cell_slots",
                 "sparse_cells", "brick_words", "mask")
MEDIUM_BOUNDS = 3
_MEDIUM_VALUE_ARRAYS = ("density", "albedo", "cells", "leaf_density", "leaf_albedo", "sparse_cells")


class DeviceMediumDesc(C.Structure):
    """cvr_device_medium_desc: a dense grid in device memory (cvr_set_medium_device)."""
    _fields_ = [("res", C.c_uint32 * 3), ("flags", C.c_uint32), ("d_density", C.c_void_p),
                ("d_albedo", C.c_void_p), ("const_albedo", C.c_float * 4), ("box_min", C.c_float * 3),
                ("box_max", C.c_float * 3), ("scale", C.c_float), ("max_density", C.c_float),
                ("g", C.c_float), ("roughness", C.c_float * 2), ("eta", C.c_float)]


SCALAR_F32, SCALAR_U8, SCALAR_U16, SCALAR_I16 = 0, 1, 2, 3
TF_CEIL, TF_DENSITY_U = 1, 2
_SCALAR_TYPES = {"float32": SCALAR_F32, "uint8": SCALAR_U8, "uint16": SCALAR_U16, "int16": SCALAR_I16}


class TransferDesc(C.Structure):
    """cvr_transfer_desc: a table of n (r, g, b, density) entries in host memory and the scalar
    range [lo, hi] it spans."""
    _fields_ = [("n", C.c_uint32), ("flags", C.c_uint32), ("table", C.c_void_p), ("lo", C.c_float),
                ("hi", C.c_float)]


class ScalarMediumDesc(C.Structure):
    """cvr_scalar_medium_desc: a scalar field in device memory and its transfer function
    (cvr_set_medium_scalar)."""
    _fields_ = [("res", C.c_uint32 * 3), ("flags", C.c_uint32), ("d_scalar", C.c_void_p),
                ("scalar_type", C.c_uint32), ("reserved", C.c_uint32), ("transfer", TransferDesc),
                ("box_min", C.c_float * 3), ("box_max", C.c_float * 3), ("scale", C.c_float),
                ("max_density", C.c_float), ("g", C.c_float), ("roughness", C.c_float * 2), ("eta", C.c_float)]


class GradientTransferDesc(C.Structure):
    """cvr_gradient_transfer_desc: a table of m rows of n (r, g, b, density) entries in host
    memory, the scalar range [lo, hi] of its rows and the gradient-magnitude range [glo, ghi] of
    its columns, and the voxel spacing the gradient is taken with."""
    _fields_ = [("n", C.c_uint32), ("m", C.c_uint32), ("flags", C.c_uint32), ("reserved", C.c_uint32),
                ("table", C.c_void_p), ("lo", C.c_float), ("hi", C.c_float), ("glo", C.c_float),
                ("ghi", C.c_float), ("spacing", C.c_float * 3)]


class GradientMediumDesc(C.Structure):
    """cvr_gradient_medium_desc: a scalar field in device memory and its gradient-magnitude
    transfer function (cvr_set_medium_gradient)."""
    _fields_ = [("res", C.c_uint32 * 3), ("flags", C.c_uint32), ("d_scalar", C.c_void_p),
                ("scalar_type", C.c_uint32), ("reserved", C.c_uint32), ("transfer", GradientTransferDesc),
                ("box_min", C.c_float * 3), ("box_max", C.c_float * 3), ("scale", C.c_float),
                ("max_density", C.c_float), ("g", C.c_float), ("roughness", C.c_float * 2), ("eta", C.c_float)]


class LabelTransferDesc(C.Structure):
    """cvr_label_transfer_desc: a table of m rows of n (r, g, b, density) entries in host memory,
    row j the transfer function of label j, and the scalar range [lo, hi] every row spans."""
    _fields_ = [("n", C.c_uint32), ("m", C.c_uint32), ("flags", C.c_uint32), ("reserved", C.c_uint32),
                ("table", C.c_void_p), ("lo", C.c_float), ("hi", C.c_float)]


class LabeledMediumDesc(C.Structure):
    """cvr_labeled_medium_desc: a scalar field and a label volume in device memory and the
    per-label transfer table (cvr_set_medium_labeled)."""
    _fields_ = [("res", C.c_uint32 * 3), ("flags", C.c_uint32), ("d_scalar", C.c_void_p),
                ("scalar_type", C.c_uint32), ("reserved", C.c_uint32), ("transfer", LabelTransferDesc),
                ("box_min", C.c_float * 3), ("box_max", C.c_float * 3), ("scale", C.c_float),
                ("max_density", C.c_float), ("g", C.c_float), ("roughness", C.c_float * 2), ("eta", C.c_float),
                ("d_labels", C.c_void_p)]


assert C.sizeof(LabelTransferDesc) == 32 and C.sizeof(LabeledMediumDesc) == 120

CLIP_MAX_PLANES = 8


class ClipDesc(C.Structure):
    """cvr_clip_desc: the crop box lo <= c < hi in voxel indices (x, y, z) and up to 8 planes
    (A, B, C, D) in voxel-index space; a voxel is kept iff the box holds it and every plane's
    ((A x + B y) + C z) + D >= 0."""
    _fields_ = [("lo", C.c_uint32 * 3), ("hi", C.c_uint32 * 3), ("n_planes", C.c_uint32), ("flags", C.c_uint32),
                ("planes", (C.c_float * 4) * CLIP_MAX_PLANES)]

    def as_dict(self):
        return {"lo": tuple(self.lo), "hi": tuple(self.hi),
                "planes": [tuple(np.float32(v) for v in self.planes[k]) for k in range(self.n_planes)]}


assert C.sizeof(ClipDesc) == 160


class FieldDesc(C.Structure):
    """cvr_field_desc: a scalar field (device memory for the Context calls, host memory for the
    *_host statements) and the voxel spacing its gradient is taken with."""
    _fields_ = [("res", C.c_uint32 * 3), ("scalar_type", C.c_uint32), ("scalar", C.c_void_p),
                ("spacing", C.c_float * 3), ("reserved", C.c_uint32)]


class FieldStatsStruct(C.Structure):
    """struct cvr_field_stats."""
    _fields_ = [("vmin", C.c_float), ("vmax", C.c_float), ("gmax", C.c_float), ("reserved", C.c_uint32),
                ("nan_values", C.c_uint64), ("nan_gradients", C.c_uint64)]


class HistogramDesc(C.Structure):
    """cvr_histogram_desc: n value bins over [lo, hi] by m gradient-magnitude bins over [glo, ghi]."""
    _fields_ = [("n", C.c_uint32), ("m", C.c_uint32), ("flags", C.c_uint32), ("reserved", C.c_uint32),
                ("lo", C.c_float), ("hi", C.c_float), ("glo", C.c_float), ("ghi", C.c_float)]


PROJECT_MAX, PROJECT_MIN, PROJECT_MEAN, PROJECT_ISO = 0, 1, 2, 3
PROJECT_HEADLIGHT = 1
_PROJECT_MODES = {"max": PROJECT_MAX, "min": PROJECT_MIN, "mean": PROJECT_MEAN, "iso": PROJECT_ISO}


class ProjectDesc(C.Structure):
    """cvr_project_desc: a projection of a raw scalar field.  mode: PROJECT_MAX, _MIN, _MEAN (shown
    through the window lo..hi) or PROJECT_ISO (the first sample >= iso, its bracket bisected
    `refine` times, lit by the field's gradient); box_min, box_max: the world box the field fills;
    step in cells of the finest axis; light: the direction towards the light (read only for ISO
    without PROJECT_HEADLIGHT); ambient, diffuse, specular, the exponent 2^shininess_log2;
    colour: the projection's full-scale colour, the surface's colour; background."""
    _fields_ = [("mode", C.c_uint32), ("flags", C.c_uint32), ("box_min", C.c_float * 3), ("box_max", C.c_float * 3),
                ("step", C.c_float), ("max_steps", C.c_uint32), ("lo", C.c_float), ("hi", C.c_float),
                ("iso", C.c_float), ("refine", C.c_uint32), ("light", C.c_float * 3), ("ambient", C.c_float),
                ("diffuse", C.c_float), ("specular", C.c_float), ("shininess_log2", C.c_uint32),
                ("colour", C.c_float * 3), ("background", C.c_float * 3), ("reserved", C.c_uint32)]

    def __init__(self, mode=PROJECT_MAX, box_min=(-0.5, -0.5, -0.5), box_max=(0.5, 0.5, 0.5), lo=0.0, hi=1.0, iso=0.5,
                 step=1.0, max_steps=4096, refine=4, light=None, ambient=0.3, diffuse=0.7, specular=0.2,
                 shininess_log2=4, colour=(1.0, 1.0, 1.0), background=(0.0, 0.0, 0.0), flags=None):
        """mode: a PROJECT_* value or "max", "min", "mean", "iso"; flags None: PROJECT_HEADLIGHT unless
        a light is given."""
        if flags is None:
            flags = PROJECT_HEADLIGHT if light is None else 0
        light = (0.0, 0.0, 0.0) if light is None else light
        f3 = lambda v: (C.c_float * 3)(*[float(x) for x in v])  # noqa: E731
        super().__init__(_PROJECT_MODES.get(mode, mode), flags, f3(box_min), f3(box_max), step, max_steps, lo, hi, iso,
                         refine, f3(light), ambient, diffuse, specular, shininess_log2, f3(colour), f3(background), 0)


assert C.sizeof(ProjectDesc) == 112


# What field_stats_host and Context.field_stats return: numpy float32 vmin, vmax, gmax (their bits
# are the library's) and the two NaN counts
FieldStats = namedtuple("FieldStats", "vmin vmax gmax nan_values nan_gradients")


class MediumLayout(C.Structure):
    """cvr_medium_layout: what an upload built (either path)."""
    _fields_ = [("sparse", C.c_uint32), ("albedo_uniform", C.c_uint32), ("n_leaves", C.c_uint32),
                ("n_cell_leaves", C.c_uint32), ("brick_shift", C.c_uint32), ("mask_shift", C.c_uint32),
                ("albedo_bg", C.c_float * 3), ("mask", C.c_uint32 * 64)]

    def as_dict(self):
        return {k: (list(getattr(self, k)) if k in ("albedo_bg", "mask") else getattr(self, k))
                for k, _ in self._fields_}


ENV_HOST, ENV_DEVICE = 0, 1


class EnvironmentDesc(C.Structure):
    """cvr_environment_desc: a latitude-longitude map of width x height texels of 3 or 4 floats in
    host or device memory, its scale and its world-to-environment rotation (all zero: identity)."""
    _fields_ = [("width", C.c_uint32), ("height", C.c_uint32), ("channels", C.c_uint32),
                ("location", C.c_uint32), ("pixels", C.c_void_p), ("scale", C.c_float),
                ("rotation", C.c_float * 9)]


class EnvironmentInfo(C.Structure):
    """cvr_environment_info: the stored map's size (0 x 0: none), device bytes and largest component."""
    _fields_ = [("width", C.c_uint32), ("height", C.c_uint32), ("bytes", C.c_uint64),
                ("max_component", C.c_float), ("reserved", C.c_uint32)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_ if k != "reserved"}


class EnvRecord(C.Structure):
    _fields_ = [("image_id", C.c_uint32), ("flags", C.c_uint32), ("n_segments", C.c_uint32),
                ("T", C.c_float * 3), ("d", C.c_float * 3), ("C", C.c_float * 3)]


ENV_RECORD_DTYPE = np.dtype([("image_id", "<u4"), ("flags", "<u4"), ("n_segments", "<u4"), ("T", "<f4", (3,)),
                             ("d", "<f4", (3,)), ("C", "<f4", (3,))])
assert ENV_RECORD_DTYPE.itemsize == C.sizeof(EnvRecord) == 48
TEXEL_FN = C.CFUNCTYPE(None, C.c_void_p, C.c_uint32, C.c_uint32, C.POINTER(C.c_float))

_lib = None


def load() -> C.CDLL:
    """Load libcvr.so (built by `make` / __graft_entry__.build()); raise if absent."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise FileNotFoundError(f"{LIB_PATH} not built: run `make` (or __graft_entry__.build())")
    lib = C.CDLL(LIB_PATH)
    P, U32, U64, I32, I64, F = C.c_void_p, C.c_uint32, C.c_uint64, C.c_int, C.c_int64, C.c_float
    FP = C.POINTER(C.c_float)
    sig = {
        "cvr_abi_version": (I32, []),
        "cvr_create": (I32, [I32, I32, C.POINTER(P)]),
        "cvr_destroy": (I32, [P]),
        "cvr_last_error": (C.c_char_p, [P]),
        "cvr_set_medium": (I32, [P, C.POINTER(MediumDesc)]),
        "cvr_set_medium_sparse": (I32, [P, C.POINTER(SparseMediumDesc)]),
        "cvr_scene_sparse_medium": (I32, [P, C.POINTER(SparseMediumDesc)]),
        "cvr_scene_is_sparse": (I32, [P]),
        "cvr_set_camera": (I32, [P, FP, FP, FP]),
        "cvr_set_resolution": (I32, [P, U32, U32]),
        "cvr_get_resolution": (I32, [P, C.POINTER(U32), C.POINTER(U32)]),
        "cvr_set_offset": (I32, [P, U32, U32]),
        "cvr_set_iterations": (I32, [P, U32]),
        "cvr_set_path_range": (I32, [P, U64, U64]),
        "cvr_set_block_shard": (I32, [P, U32, U32]),
        "cvr_set_block_order": (I32, [P, P, U32]),
        "cvr_share_medium": (I32, [P, P]),
        "cvr_medium_info": (I32, [P, C.POINTER(MediumInfo)]),
        "cvr_half_round": (I32, [FP, FP, C.c_size_t]),
        "cvr_trace_launch": (I32, [P, P, U64]),
        "cvr_image_to_host": (I32, [P, P, C.c_size_t, C.c_float, P]),
        "cvr_render_frame": (I32, [P, P, C.c_size_t, U32, C.POINTER(Stats)]),
        "cvr_frame_flush_info": (I32, [P, C.POINTER(U32), C.POINTER(U32)]),
        "cvr_blocks_to_host": (I32, [P, P, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_float, P]),
        "cvr_launch_blocks": (I32, [P, P, P, P]),
        "cvr_set_seed": (I32, [P, U32]),
        "cvr_get_seed": (I32, [P, C.POINTER(U32)]),
        "cvr_set_output": (I32, [P, P]),
        "cvr_output_ptr": (P, [P]),
        "cvr_set_stream": (I32, [P, P]),
        "cvr_own_stream": (P, [P]),
        "cvr_set_option": (I32, [P, I32, I64]),
        "cvr_init": (I32, [P]),
        "cvr_launch_render": (I32, [P]),
        "cvr_reset": (I32, [P]),
        "cvr_synchronize": (I32, [P]),
        "cvr_clear_output": (I32, [P]),
        "cvr_get_stats": (I32, [P, C.POINTER(Stats)]),
        "cvr_copy_output": (I32, [P, FP, F]),
        "cvr_trace_paths": (I32, [P, U32, U32, C.POINTER(PathRecord)]),
        "cvr_device_info": (I32, [P, C.POINTER(I32), C.POINTER(I32)]),
        "cvr_render_image": (I32, [P, C.POINTER(RenderDesc), P, FP, C.POINTER(Stats)]),
        "cvr_render_tiles": (I32, [P, C.POINTER(RenderDesc), U32, U32, P, FP, C.POINTER(Stats)]),
        "cvr_render_share_to_host": (I32, [P, C.POINTER(RenderDesc), U32, U32, P, C.c_size_t, C.POINTER(Stats)]),
        "cvr_host_alloc": (I32, [C.c_size_t, C.POINTER(C.c_void_p)]),
        "cvr_host_free": (I32, [P]),
        "cvr_default_camera": (I32, [U32, U32, FP, FP]),
        "cvr_tiling": (I32, [U32, U32, U32, U32, C.POINTER(U32)]),
        "cvr_tile_origin": (I32, [U32, U32, C.POINTER(U32), C.POINTER(U32)]),
        "cvr_scene_load": (I32, [C.c_char_p, I32, C.POINTER(P)]),
        "cvr_scene_load_ex": (I32, [C.c_char_p, I32, C.POINTER(LoadOptions), C.POINTER(P)]),
        "cvr_scene_synthetic": (I32, [C.c_char_p, U32, C.POINTER(U32), C.POINTER(P)]),
        "cvr_scene_medium": (I32, [P, C.POINTER(MediumDesc)]),
        "cvr_scene_camera": (I32, [P, U32, U32, P, P]),
        "cvr_scene_raw_bytes": (I32, [P, C.POINTER(C.POINTER(C.c_uint8)), C.POINTER(C.c_size_t)]),
        "cvr_scene_destroy": (None, [P]),
        "cvr_write_hdr": (I32, [C.c_char_p, FP, U32, U32]),
        "cvr_kernel_from_name": (I32, [C.c_char_p]),
        "cvr_kernel_name": (C.c_char_p, [I32]),
        "cvr_copy_moments": (I32, [P, FP, FP]),
        "cvr_block_error": (I32, [FP, FP, U32, U32, F, C.POINTER(C.c_double)]),
        "cvr_adaptive_begin": (I32, [P, C.POINTER(AdaptiveDesc)]),
        "cvr_adaptive_pass": (I32, [P, C.POINTER(AdaptiveResult)]),
        "cvr_adaptive_maps": (I32, [P, C.POINTER(C.c_double), C.POINTER(U32)]),
        "cvr_adaptive_image": (I32, [P, P, C.c_size_t]),
        "cvr_adaptive_end": (I32, [P]),
        "cvr_render_adaptive": (I32, [P, C.POINTER(AdaptiveDesc), P, C.c_size_t, C.POINTER(AdaptiveResult),
                                      C.POINTER(Stats)]),
        "cvr_denoise_host": (I32, [P, P, U32, U32, U32, P, C.POINTER(DenoiseDesc), P, P]),
        "cvr_denoise_buffers": (I32, [P, P, P, U32, U32, U32, P, C.POINTER(DenoiseDesc), P, P]),
        "cvr_denoise": (I32, [P, C.POINTER(DenoiseDesc), U32, P, C.c_size_t]),
        "cvr_features_host": (I32, [C.POINTER(MediumDesc), FP, FP, FP, U32, U32, U32, U32, I32, C.POINTER(FeaturesDesc),
                                    P, P]),
        "cvr_features_buffers": (I32, [P, C.POINTER(FeaturesDesc), P, P]),
        "cvr_features": (I32, [P, C.POINTER(FeaturesDesc), P, P, C.c_size_t]),
        "cvr_preview_host": (I32, [C.POINTER(MediumDesc), FP, FP, FP, U32, U32, U32, U32, I32, C.POINTER(PreviewDesc), P]),
        "cvr_preview_buffers": (I32, [P, C.POINTER(PreviewDesc), P]),
        "cvr_preview": (I32, [P, C.POINTER(PreviewDesc), P, C.c_size_t]),
        "cvr_light_volume_host": (I32, [C.POINTER(MediumDesc), I32, C.POINTER(LightVolumeDesc), P]),
        "cvr_build_light_volume": (I32, [P, C.POINTER(LightVolumeDesc)]),
        "cvr_light_volume_default_res": (I32, [P, C.POINTER(U32)]),
        "cvr_light_volume_info": (I32, [P, C.POINTER(LightVolumeInfo)]),
        "cvr_copy_light_volume": (I32, [P, P, C.c_size_t]),
        "cvr_clear_light_volume": (I32, [P]),
        "cvr_preview_shadowed_host": (I32, [C.POINTER(MediumDesc), FP, FP, FP, U32, U32, U32, U32, I32,
                                            C.POINTER(PreviewDesc), C.POINTER(LightVolumeDesc), P, C.c_float, P]),
        "cvr_preview_shadowed_buffers": (I32, [P, C.POINTER(PreviewDesc), C.c_float, P]),
        "cvr_preview_shadowed": (I32, [P, C.POINTER(PreviewDesc), C.c_float, P, C.c_size_t]),
        "cvr_denoise_guided_host": (I32, [P, P, U32, U32, U32, P, C.POINTER(DenoiseGuidedDesc), P, P, P, P]),
        "cvr_denoise_guided_buffers": (I32, [P, P, P, U32, U32, U32, P, C.POINTER(DenoiseGuidedDesc), P, P, P, P]),
        "cvr_denoise_guided": (I32, [P, C.POINTER(DenoiseGuidedDesc), C.POINTER(FeaturesDesc), U32, P, C.c_size_t]),
        "cvr_set_medium_device": (I32, [P, C.POINTER(DeviceMediumDesc)]),
        "cvr_medium_layout": (I32, [P, C.POINTER(MediumLayout)]),
        "cvr_debug_device_medium_ms": (I32, [P, C.POINTER(C.c_double)]),
        "cvr_debug_copy_medium": (I32, [P, I32, P, C.c_size_t, C.POINTER(C.c_size_t)]),
        "cvr_debug_build_geometry": (I32, [C.POINTER(U32)]),
        "cvr_classify_host": (I32, [P, U32, C.c_size_t, C.POINTER(TransferDesc), P, P]),
        "cvr_raw_transfer_table": (I32, [FP]),
        "cvr_set_medium_scalar": (I32, [P, C.POINTER(ScalarMediumDesc)]),
        "cvr_set_medium_scene_transfer": (I32, [P, P, C.POINTER(TransferDesc), U32]),
        "cvr_classify_gradient_host": (I32, [P, U32, C.POINTER(U32), C.POINTER(GradientTransferDesc), P, P, P]),
        "cvr_set_medium_gradient": (I32, [P, C.POINTER(GradientMediumDesc)]),
        "cvr_set_medium_scene_gradient": (I32, [P, P, C.POINTER(GradientTransferDesc), U32]),
        "cvr_classify_labels_host": (I32, [P, U32, P, C.c_size_t, C.POINTER(LabelTransferDesc), P, P, P]),
        "cvr_set_medium_labeled": (I32, [P, C.POINTER(LabeledMediumDesc)]),
        "cvr_medium_label_info": (I32, [P, C.POINTER(U32), C.POINTER(U64)]),
        "cvr_set_medium_scene_labels": (I32, [P, P, C.POINTER(LabelTransferDesc), P, C.c_size_t, U32]),
        "cvr_set_clip": (I32, [P, C.POINTER(ClipDesc)]),
        "cvr_clear_clip": (I32, [P]),
        "cvr_get_clip": (I32, [P, C.POINTER(ClipDesc), C.POINTER(I32)]),
        "cvr_clip_host": (I32, [C.POINTER(U32), C.POINTER(ClipDesc), P, P, P]),
        "cvr_medium_clip_info": (I32, [P, C.POINTER(ClipDesc), C.POINTER(U64)]),
        "cvr_field_stats_host": (I32, [C.POINTER(FieldDesc), C.POINTER(FieldStatsStruct)]),
        "cvr_field_histogram_host": (I32, [C.POINTER(FieldDesc), C.POINTER(HistogramDesc), P]),
        "cvr_field_stats": (I32, [P, C.POINTER(FieldDesc), C.POINTER(FieldStatsStruct)]),
        "cvr_field_histogram": (I32, [P, C.POINTER(FieldDesc), C.POINTER(HistogramDesc), P]),
        "cvr_field_histogram_buffers": (I32, [P, C.POINTER(FieldDesc), C.POINTER(HistogramDesc), P]),
        "cvr_field_project_host": (I32, [C.POINTER(FieldDesc), C.POINTER(ProjectDesc), FP, FP, FP, U32, U32, U32, U32, P, P, P]),
        "cvr_field_project_buffers": (I32, [P, C.POINTER(FieldDesc), C.POINTER(ProjectDesc), P, P, P]),
        "cvr_field_project": (I32, [P, C.POINTER(FieldDesc), C.POINTER(ProjectDesc), P, P, P, C.c_size_t]),
        "cvr_debug_field_geometry": (I32, [C.POINTER(U32)]),
        "cvr_set_environment": (I32, [P, C.POINTER(EnvironmentDesc)]),
        "cvr_clear_environment": (I32, [P]),
        "cvr_environment_info": (I32, [P, C.POINTER(EnvironmentInfo)]),
        "cvr_environment_eval_host": (I32, [C.POINTER(EnvironmentDesc), FP, C.c_size_t, FP]),
        "cvr_environment_eval_host_fn": (I32, [U32, U32, FP, TEXEL_FN, P, FP, C.c_size_t, FP]),
        "cvr_environment_eval": (I32, [P, FP, C.c_size_t, FP]),
        "cvr_trace_env": (I32, [P, U32, U32, C.POINTER(EnvRecord)]),
        "cvr_read_image": (I32, [C.c_char_p, C.POINTER(U32), C.POINTER(U32), C.POINTER(FP)]),
        "cvr_free_image": (None, [FP]),
        "cvr_debug_wpool_rows": (I32, [C.POINTER(C.c_int32), U32, C.POINTER(U32)]),
        "cvr_debug_last_wpool": (I32, [P, C.POINTER(C.c_int32), C.POINTER(U32)]),
    }
    # an older experiment build (tools' --lib, A/B against a previous commit) may lack newer entry
    # points; the in-tree library must export every one (tests/test_host_abi.py)
    older_ok = os.path.abspath(LIB_PATH) != _DEFAULT_LIB
    for name, (res, args) in sig.items():
        if older_ok and not hasattr(lib, name):
            continue
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


def _fp(a: np.ndarray):
    return a.ctypes.data_as(C.POINTER(C.c_float))


def _check(code: int, ctx=None):
    if code != CVR_OK:
        msg = load().cvr_last_error(ctx)
        raise CvrError(code, msg.decode() if msg else "")


# ------------------------------------------------------------------ helpers --
def half_round(a) -> np.ndarray:
    """f32 -> IEEE binary16 (nearest even, subnormals kept) -> f32, the rounding of OPT_MEDIUM_FORMAT
    FORMAT_F16 (cvr_half_round; host only): a FORMAT_F16 render is bit-identical per path to a
    FORMAT_F32 render of the half_round()ed arrays."""
    src = np.ascontiguousarray(a, dtype=np.float32)
    out = np.empty_like(src)
    _check(load().cvr_half_round(_fp(src), _fp(out), src.size))
    return out


def block_error(sum_rgba, m2_rgba, n_samples: int, floor: float) -> float:
    """The adaptive render's noise metric (cvr_block_error; host only): the mean over the given
    pixels (an 8x8 block) of the relative standard error of the pixel's mean, from the raw sums
    `sum_rgba` (framebuffer) and `m2_rgba` (moments), (..., 4) floats each, n_samples per pixel."""
    a = np.ascontiguousarray(sum_rgba, dtype=np.float32).reshape(-1, 4)
    b = np.ascontiguousarray(m2_rgba, dtype=np.float32).reshape(-1, 4)
    if a.shape != b.shape:
        raise CvrError(-1, "block_error: sum and m2 differ in shape")
    out = C.c_double()
    _check(load().cvr_block_error(_fp(a), _fp(b), a.shape[0], n_samples, floor, C.byref(out)))
    return out.value


def denoise_host(sum_rgba, m2_rgba, n_samples: Optional[int] = None, block_samples=None,
                 desc: Optional[DenoiseDesc] = None):
    """The denoiser's written statement on the CPU (cvr_denoise_host; no GPU): the raw sums
    `sum_rgba` and second moments `m2_rgba`, (h, w, 4) floats each (Context.copy_moments), with
    n_samples per pixel or a (h / 8, w / 8) map of per-block counts -> (rgba (h, w, 4), var (h, w)):
    the filtered image (w: the pixel's escapes per sample) and the filtered variance of the pixel
    mean's luminance, -1 where no valid pixel reached.  The device paths return the same bits."""
    s1 = np.ascontiguousarray(sum_rgba, dtype=np.float32)
    s2 = np.ascontiguousarray(m2_rgba, dtype=np.float32)
    if s1.ndim != 3 or s1.shape[2] != 4 or s1.shape != s2.shape:
        raise CvrError(-1, "denoise_host: sum and m2 must both be (h, w, 4)")
    h, w = s1.shape[:2]
    counts = None
    if block_samples is not None:
        counts = np.ascontiguousarray(block_samples, dtype=np.uint32)
        if counts.size != (h // 8) * (w // 8):
            raise CvrError(-1, "denoise_host: block_samples must hold (h / 8) * (w / 8) counts")
    desc = DenoiseDesc() if desc is None else desc
    rgba = np.zeros((h, w, 4), np.float32)
    var = np.zeros((h, w), np.float32)
    _check(load().cvr_denoise_host(s1.ctypes.data, s2.ctypes.data, w, h, n_samples or 0,
                                   None if counts is None else counts.ctypes.data, C.byref(desc), rgba.ctypes.data,
                                   var.ctypes.data))
    return rgba, var


def denoise_guided_host(sum_rgba, m2_rgba, feat_rgba, feat_depth, n_samples: Optional[int] = None, block_samples=None,
                        desc: Optional[DenoiseGuidedDesc] = None):
    """The feature-guided filter's written statement on the CPU (cvr_denoise_guided_host; no GPU):
    denoise_host's arguments plus the feature planes feat_rgba (h, w, 4) and feat_depth (h, w)
    (features_host, Context.features) -> (rgba, var) as denoise_host.  With every sigma of `desc`
    <= 0 the bits are denoise_host's."""
    s1 = np.ascontiguousarray(sum_rgba, dtype=np.float32)
    s2 = np.ascontiguousarray(m2_rgba, dtype=np.float32)
    if s1.ndim != 3 or s1.shape[2] != 4 or s1.shape != s2.shape:
        raise CvrError(-1, "denoise_guided_host: sum and m2 must both be (h, w, 4)")
    h, w = s1.shape[:2]
    f4 = np.ascontiguousarray(feat_rgba, dtype=np.float32)
    fz = np.ascontiguousarray(feat_depth, dtype=np.float32)
    if f4.shape != (h, w, 4) or fz.shape != (h, w):
        raise CvrError(-1, "denoise_guided_host: feat_rgba must be (h, w, 4) and feat_depth (h, w)")
    counts = None
    if block_samples is not None:
        counts = np.ascontiguousarray(block_samples, dtype=np.uint32)
        if counts.size != (h // 8) * (w // 8):
            raise CvrError(-1, "denoise_guided_host: block_samples must hold (h / 8) * (w / 8) counts")
    desc = DenoiseGuidedDesc() if desc is None else desc
    rgba = np.zeros((h, w, 4), np.float32)
    var = np.zeros((h, w), np.float32)
    _check(load().cvr_denoise_guided_host(s1.ctypes.data, s2.ctypes.data, w, h, n_samples or 0,
                                          None if counts is None else counts.ctypes.data, C.byref(desc), f4.ctypes.data,
                                          fz.ctypes.data, rgba.ctypes.data, var.ctypes.data))
    return rgba, var


def features_host(medium: "MediumDesc", inv_view, raster_to_view, full_res, tile=None, offset=(0, 0),
                  world_to_aabb: int = 0, desc: Optional[FeaturesDesc] = None):
    """The feature pass's written statement on the CPU (cvr_features_host; no GPU) on a dense
    medium's host arrays, for tile (w, h) (default: full_res) at `offset` of the full image ->
    (feat_rgba (h, w, 4): mean first-collision albedo and opacity, feat_depth (h, w): mean
    collision depth over the box diagonal).  Context.features returns the same bits."""
    iv = np.ascontiguousarray(inv_view, dtype=np.float32).reshape(12)
    r2v = np.ascontiguousarray(raster_to_view, dtype=np.float32).reshape(2)
    fr = np.asarray(full_res, dtype=np.float32).reshape(2)
    w, h = (int(full_res[0]), int(full_res[1])) if tile is None else (int(tile[0]), int(tile[1]))
    desc = FeaturesDesc() if desc is None else desc
    rgba = np.zeros((max(h, 0), max(w, 0), 4), np.float32)
    depth = np.zeros((max(h, 0), max(w, 0)), np.float32)
    _check(load().cvr_features_host(C.byref(medium), _fp(iv), _fp(r2v), _fp(fr), w, h, int(offset[0]), int(offset[1]),
                                    int(world_to_aabb), C.byref(desc), rgba.ctypes.data, depth.ctypes.data))
    return rgba, depth


def preview_host(medium: "MediumDesc", inv_view, raster_to_view, full_res, tile=None, offset=(0, 0),
                 world_to_aabb: int = 0, desc: Optional[PreviewDesc] = None) -> np.ndarray:
    """The shaded preview's written statement on the CPU (cvr_preview_host; no GPU) on a dense
    medium's host arrays, features_host's arguments -> rgba (h, w, 4): the composited colour over
    the background and the opacity.  Context.preview returns the same bits."""
    iv = np.ascontiguousarray(inv_view, dtype=np.float32).reshape(12)
    r2v = np.ascontiguousarray(raster_to_view, dtype=np.float32).reshape(2)
    fr = np.asarray(full_res, dtype=np.float32).reshape(2)
    w, h = (int(full_res[0]), int(full_res[1])) if tile is None else (int(tile[0]), int(tile[1]))
    desc = PreviewDesc() if desc is None else desc
    rgba = np.zeros((max(h, 0), max(w, 0), 4), np.float32)
    _check(load().cvr_preview_host(C.byref(medium), _fp(iv), _fp(r2v), _fp(fr), w, h, int(offset[0]), int(offset[1]),
                                   int(world_to_aabb), C.byref(desc), rgba.ctypes.data))
    return rgba


def light_volume_host(medium: "MediumDesc", desc: LightVolumeDesc, world_to_aabb: int = 0) -> np.ndarray:
    """The light volume's written statement on the CPU (cvr_light_volume_host; no GPU) on a dense
    medium's host arrays -> the transmittances (z, y, x) of desc.res.  Context.light_volume returns
    the same bits."""
    out = np.zeros(tuple(int(v) for v in desc.res)[::-1], np.float32)
    _check(load().cvr_light_volume_host(C.byref(medium), int(world_to_aabb), C.byref(desc), out.ctypes.data))
    return out


def preview_shadowed_host(medium: "MediumDesc", inv_view, raster_to_view, full_res, volume_desc: LightVolumeDesc,
                          volume, tile=None, offset=(0, 0), world_to_aabb: int = 0,
                          desc: Optional[PreviewDesc] = None, shadow: float = 0.7) -> np.ndarray:
    """The shadowed preview's written statement on the CPU (cvr_preview_shadowed_host; no GPU):
    preview_host's arguments plus the light volume (light_volume_host's array and its descriptor)
    and the shadow strength -> rgba (h, w, 4).  desc None: the default shading without the
    headlight; its light is not read (the volume's is).  Context.preview_shadowed returns the same bits."""
    iv = np.ascontiguousarray(inv_view, dtype=np.float32).reshape(12)
    r2v = np.ascontiguousarray(raster_to_view, dtype=np.float32).reshape(2)
    fr = np.asarray(full_res, dtype=np.float32).reshape(2)
    w, h = (int(full_res[0]), int(full_res[1])) if tile is None else (int(tile[0]), int(tile[1]))
    desc = PreviewDesc(flags=0) if desc is None else desc
    vol = np.ascontiguousarray(volume, dtype=np.float32)
    if vol.shape != tuple(int(v) for v in volume_desc.res)[::-1]:
        raise CvrError(-1, f"preview_shadowed_host: volume {vol.shape}, expected (z, y, x) of res {tuple(volume_desc.res)}")
    rgba = np.zeros((max(h, 0), max(w, 0), 4), np.float32)
    _check(load().cvr_preview_shadowed_host(C.byref(medium), _fp(iv), _fp(r2v), _fp(fr), w, h, int(offset[0]),
                                            int(offset[1]), int(world_to_aabb), C.byref(desc), C.byref(volume_desc),
                                            vol.ctypes.data, float(shadow), rgba.ctypes.data))
    return rgba


def _transfer_desc(table, lo, hi, ceil, density_u):
    """(TransferDesc, the array it points into): table is (n, 4) floats (r, g, b, density)."""
    tab = np.ascontiguousarray(table, dtype=np.float32)
    if tab.ndim != 2 or tab.shape[1] != 4:
        raise ValueError(f"table: shape {tab.shape}, expected (n, 4)")
    t = TransferDesc(tab.shape[0], (TF_CEIL if ceil else 0) | (TF_DENSITY_U if density_u else 0), tab.ctypes.data,
                     lo, hi)
    return t, tab


def classify_host(scalar, table, lo, hi, ceil=False, density_u=False):
    """The transfer function's written statement on the CPU (cvr_classify_host; no GPU): a numpy
    array `scalar` of dtype uint8, uint16, int16 or float32 and a table of (n, 4) floats
    (r, g, b, density) over the scalar range [lo, hi] -> (density scalar.shape, albedo
    scalar.shape + (4,)).  ceil: entry ceil(x) instead of linear interpolation; density_u: the
    density is the normalised scalar, not the table's.  Context.set_medium_scalar computes the same
    bits on the device."""
    src = np.ascontiguousarray(scalar)
    if src.dtype.name not in _SCALAR_TYPES:
        raise ValueError(f"scalar: dtype {src.dtype}, expected uint8, uint16, int16 or float32")
    t, _tab = _transfer_desc(table, lo, hi, ceil, density_u)
    density = np.empty(src.shape, np.float32)
    albedo = np.empty(src.shape + (4,), np.float32)
    _check(load().cvr_classify_host(src.ctypes.data, _SCALAR_TYPES[src.dtype.name], src.size, C.byref(t),
                                    density.ctypes.data, albedo.ctypes.data))
    return density, albedo


def _gradient_transfer_desc(table, lo, hi, glo, ghi, spacing):
    """(GradientTransferDesc, the array it points into): table is (m, n, 4) floats, row j the
    gradient entry j."""
    tab = np.ascontiguousarray(table, dtype=np.float32)
    if tab.ndim != 3 or tab.shape[2] != 4:
        raise ValueError(f"table: shape {tab.shape}, expected (m, n, 4)")
    if len(spacing) != 3:
        raise ValueError("spacing: expected 3 floats (x, y, z)")
    t = GradientTransferDesc(tab.shape[1], tab.shape[0], 0, 0, tab.ctypes.data, lo, hi, glo, ghi)
    t.spacing[:] = [float(v) for v in spacing]
    return t, tab


def classify_gradient_host(scalar, table, lo, hi, glo, ghi, spacing=(1.0, 1.0, 1.0)):
    """The gradient-magnitude transfer function's written statement on the CPU
    (cvr_classify_gradient_host; no GPU): a (z, y, x) numpy array `scalar` of dtype uint8, uint16,
    int16 or float32 and a table of (m, n, 4) floats (r, g, b, density), its n columns over the
    scalar range [lo, hi] and its m rows over the gradient-magnitude range [glo, ghi], the
    gradient taken with voxel spacing (x, y, z) -> (density (z, y, x), albedo (z, y, x, 4),
    gradient magnitude (z, y, x)).  Context.set_medium_gradient computes the same bits on the
    device."""
    src = np.ascontiguousarray(scalar)
    if src.dtype.name not in _SCALAR_TYPES:
        raise ValueError(f"scalar: dtype {src.dtype}, expected uint8, uint16, int16 or float32")
    if src.ndim != 3:
        raise ValueError(f"scalar: shape {src.shape}, expected (z, y, x)")
    t, _tab = _gradient_transfer_desc(table, lo, hi, glo, ghi, spacing)
    density = np.empty(src.shape, np.float32)
    albedo = np.empty(src.shape + (4,), np.float32)
    mag = np.empty(src.shape, np.float32)
    res = (C.c_uint32 * 3)(src.shape[2], src.shape[1], src.shape[0])
    _check(load().cvr_classify_gradient_host(src.ctypes.data, _SCALAR_TYPES[src.dtype.name], res, C.byref(t),
                                             density.ctypes.data, albedo.ctypes.data, mag.ctypes.data))
    return density, albedo, mag


def _label_transfer_desc(table, lo, hi, ceil, density_u):
    """(LabelTransferDesc, the array it points into): table is (m, n, 4) floats, row j the
    transfer function of label j."""
    tab = np.ascontiguousarray(table, dtype=np.float32)
    if tab.ndim != 3 or tab.shape[2] != 4:
        raise ValueError(f"table: shape {tab.shape}, expected (m, n, 4)")
    t = LabelTransferDesc(tab.shape[1], tab.shape[0], (TF_CEIL if ceil else 0) | (TF_DENSITY_U if density_u else 0), 0,
                          tab.ctypes.data, lo, hi)
    return t, tab


def classify_labels_host(scalar, labels, table, lo, hi, ceil=False, density_u=False):
    """The labelled classification's written statement on the CPU (cvr_classify_labels_host; no
    GPU): a numpy array `scalar` of dtype uint8, uint16, int16 or float32, a uint8 array `labels`
    of the same element count and a table of (m, n, 4) floats (r, g, b, density), row j the
    transfer function of label j over the scalar range [lo, hi] (a label byte >= m takes row 0)
    -> (density scalar.shape, albedo scalar.shape + (4,), counts: 256 uint64, the voxels with
    each label byte).  ceil and density_u are classify_host's.  Context.set_medium_labeled
    computes the same bits on the device."""
    src = np.ascontiguousarray(scalar)
    if src.dtype.name not in _SCALAR_TYPES:
        raise ValueError(f"scalar: dtype {src.dtype}, expected uint8, uint16, int16 or float32")
    lab = np.ascontiguousarray(labels)
    if lab.dtype != np.uint8 or lab.size != src.size:
        raise ValueError(f"labels: dtype {lab.dtype}, {lab.size} elements, expected uint8 and {src.size}")
    t, _tab = _label_transfer_desc(table, lo, hi, ceil, density_u)
    density = np.empty(src.shape, np.float32)
    albedo = np.empty(src.shape + (4,), np.float32)
    counts = np.zeros(256, np.uint64)
    _check(load().cvr_classify_labels_host(src.ctypes.data, _SCALAR_TYPES[src.dtype.name], lab.ctypes.data, src.size,
                                           C.byref(t), density.ctypes.data, albedo.ctypes.data, counts.ctypes.data))
    return density, albedo, counts


def _clip_desc(lo=None, hi=None, planes=()) -> ClipDesc:
    """The descriptor of a crop box (lo, hi: (x, y, z) voxel indices, None: no bound) and planes
    ((A, B, C, D) each).  More than 8 planes are passed on for the library to refuse."""
    planes = [tuple(float(v) for v in p) for p in planes]
    if any(len(p) != 4 for p in planes):
        raise ValueError("planes: expected (A, B, C, D) each")
    d = ClipDesc()
    d.lo[:] = [int(v) for v in (lo if lo is not None else (0, 0, 0))]
    d.hi[:] = [min(int(v), 0xFFFFFFFF) for v in (hi if hi is not None else (0xFFFFFFFF,) * 3)]
    d.n_planes = len(planes)
    for k, p in enumerate(planes[:CLIP_MAX_PLANES]):
        d.planes[k][:] = p
    return d


def clip_host(res, lo=None, hi=None, planes=(), density=None, albedo=None):
    """The clip region's written statement on the CPU (cvr_clip_host; no GPU) for a grid of
    res = (nx, ny, nz) voxels: -> (keep (z, y, x) uint8, density, albedo), the two arrays copies of
    the given ones ((z, y, x) and (z, y, x, 4) float32; None stays None) with every clipped voxel
    set to density 0 and voxel (0, 0, 0)'s albedo.  The device builds of a Context with the same
    set_clip store exactly these values."""
    nx, ny, nz = (int(v) for v in res)
    d = _clip_desc(lo, hi, planes)
    keep = np.empty((nz, ny, nx), np.uint8)
    dn = al = None
    if density is not None:
        dn = np.array(density, dtype=np.float32, order="C", copy=True)
        if dn.shape != (nz, ny, nx):
            raise ValueError(f"density: shape {dn.shape}, expected {(nz, ny, nx)}")
    if albedo is not None:
        al = np.array(albedo, dtype=np.float32, order="C", copy=True)
        if al.shape != (nz, ny, nx, 4):
            raise ValueError(f"albedo: shape {al.shape}, expected {(nz, ny, nx, 4)}")
    r = (C.c_uint32 * 3)(nx, ny, nz)
    _check(load().cvr_clip_host(r, C.byref(d), dn.ctypes.data if dn is not None else None,
                                al.ctypes.data if al is not None else None, keep.ctypes.data))
    return keep, dn, al


def plane_from_box(point, normal, box_min, box_max, res):
    """A clip plane given by a point on it and its normal in box coordinates (the side the normal
    points to is kept) -> (A, B, C, D) float32 in voxel-index space for a grid of res = (nx, ny,
    nz) voxels in the box [box_min, box_max], voxel index i_a = (p_a - min_a) / extent_a *
    (res_a - 1).  An axis of one voxel has no extent in index space: its coefficient is 0."""
    p, n = np.asarray(point, np.float64), np.asarray(normal, np.float64)
    lo, hi = np.asarray(box_min, np.float64), np.asarray(box_max, np.float64)
    cells = np.asarray(res, np.float64) - 1.0
    if p.shape != (3,) or n.shape != (3,) or lo.shape != (3,) or hi.shape != (3,) or cells.shape != (3,):
        raise ValueError("plane_from_box: point, normal, box_min, box_max and res are 3 numbers each")
    # p_a = min_a + i_a * extent_a / cells_a, so n . (p - point) = sum_a n_a extent_a / cells_a * i_a + n . (min - point)
    abc = np.where(cells > 0.0, n * (hi - lo) / np.where(cells > 0.0, cells, 1.0), 0.0)
    dd = float(np.dot(n, lo - p))
    return tuple(np.float32(v) for v in (abc[0], abc[1], abc[2], dd))


def build_geometry() -> dict:
    """The launch geometry of the medium build kernels (cvr_debug_build_geometry; no GPU needed),
    by name."""
    out = (C.c_uint32 * 16)()
    _check(load().cvr_debug_build_geometry(out))
    names = ("scan_grid", "stream_grid", "scan_tile", "scan_sums_chunk", "gradient_tasks", "gradient_z",
             "leaf_run_voxels", "leaf_run_leaves", "leaf_flags_grid", "to_half_grid", "cells_grid", "bounds_grid",
             "sparse_cells_grid", "sparse_bounds_grid")
    if out[15] != len(names):
        raise RuntimeError(f"cvr_debug_build_geometry fills {out[15]} entries, this binding knows {len(names)}")
    return dict(zip(names, (int(v) for v in out)))


def wpool_rows() -> list:
    """The wave-pool kernel instances the library ships, in table order, as (eps, waves, med, record,
    flush) tuples of ints (cvr_debug_wpool_rows; no GPU needed)."""
    n = C.c_uint32(0)
    _check(load().cvr_debug_wpool_rows(None, 0, C.byref(n)))
    rows = (C.c_int32 * (5 * n.value))()
    _check(load().cvr_debug_wpool_rows(rows, n.value, C.byref(n)))
    return [tuple(int(v) for v in rows[5 * i:5 * i + 5]) for i in range(n.value)]


def field_geometry() -> dict:
    """The launch geometry of the field kernels (cvr_debug_field_geometry; no GPU needed), by name."""
    out = (C.c_uint32 * 8)()
    _check(load().cvr_debug_field_geometry(out))
    names = ("walk_tasks", "walk_z", "hist1d_grid", "lds_bins", "max_bins")
    if out[7] != len(names):
        raise RuntimeError(f"cvr_debug_field_geometry fills {out[7]} entries, this binding knows {len(names)}")
    return dict(zip(names, (int(v) for v in out)))


def _field_desc(ptr, scalar_type, res, spacing):
    if len(spacing) != 3:
        raise ValueError("spacing: expected 3 floats (x, y, z)")
    f = FieldDesc()
    f.res[:] = [int(v) for v in res]
    f.scalar_type = scalar_type
    f.scalar = ptr
    f.spacing[:] = [float(v) for v in spacing]
    return f


def _histogram_desc(n, m, lo, hi, glo, ghi):
    if m > 1 and (glo is None or ghi is None):
        raise ValueError("field_histogram: glo and ghi are required with m > 1")
    return HistogramDesc(n, m, 0, 0, lo, hi, 0.0 if glo is None else glo, 0.0 if ghi is None else ghi)


def _field_stats(st: "FieldStatsStruct") -> "FieldStats":
    return FieldStats(np.float32(st.vmin), np.float32(st.vmax), np.float32(st.gmax), int(st.nan_values),
                      int(st.nan_gradients))


def _host_field(scalar, spacing):
    src = np.ascontiguousarray(scalar)
    if src.dtype.name not in _SCALAR_TYPES:
        raise ValueError(f"scalar: dtype {src.dtype}, expected uint8, uint16, int16 or float32")
    if src.ndim != 3:
        raise ValueError(f"scalar: shape {src.shape}, expected (z, y, x)")
    return src, _field_desc(src.ctypes.data, _SCALAR_TYPES[src.dtype.name], src.shape[::-1], spacing)


def field_stats_host(scalar, spacing=(1.0, 1.0, 1.0)) -> "FieldStats":
    """The field statistics' written statement on the CPU (cvr_field_stats_host; no GPU): of a
    (z, y, x) numpy array of dtype uint8, uint16, int16 or float32, the smallest and largest
    non-NaN value, the largest non-NaN gradient magnitude (the gradient of
    classify_gradient_host, with voxel spacing (x, y, z)) and the counts of NaN values and NaN
    magnitudes.  Context.field_stats returns the same bits from the device."""
    _src, f = _host_field(scalar, spacing)
    st = FieldStatsStruct()
    _check(load().cvr_field_stats_host(C.byref(f), C.byref(st)))
    return _field_stats(st)


def field_histogram_host(scalar, n, m=1, *, lo, hi, glo=None, ghi=None, spacing=(1.0, 1.0, 1.0)) -> np.ndarray:
    """The histogram's written statement on the CPU (cvr_field_histogram_host; no GPU): the (m, n)
    uint32 counts of the voxels of a (z, y, x) numpy array nearest each node of a table of m rows
    (gradient magnitude over [glo, ghi]) of n entries (value over [lo, hi]).  m = 1: the 1-D
    histogram, no gradient.  Context.field_histogram returns the same counts from the device."""
    _src, f = _host_field(scalar, spacing)
    h = _histogram_desc(n, m, lo, hi, glo, ghi)
    counts = np.empty((max(int(m), 0), max(int(n), 0)), np.uint32)
    _check(load().cvr_field_histogram_host(C.byref(f), C.byref(h), counts.ctypes.data))
    return counts


def field_project_host(scalar, inv_view, raster_to_view, full_res, desc: Optional[ProjectDesc] = None, tile=None,
                       offset=(0, 0)):
    """The field projections' written statement on the CPU (cvr_field_project_host; no GPU): of a
    (z, y, x) numpy array of dtype uint8, uint16, int16 or float32 filling desc's box, for tile
    (w, h) (default: full_res) at `offset` of the full image -> (rgba (h, w, 4), value (h, w): the
    projected or the surface's field value, depth (h, w): its distance over the box diagonal).
    Context.field_project returns the same bits from the device."""
    _src, f = _host_field(scalar, (1.0, 1.0, 1.0))
    iv = np.ascontiguousarray(inv_view, dtype=np.float32).reshape(12)
    r2v = np.ascontiguousarray(raster_to_view, dtype=np.float32).reshape(2)
    fr = np.asarray(full_res, dtype=np.float32).reshape(2)
    w, h = (int(full_res[0]), int(full_res[1])) if tile is None else (int(tile[0]), int(tile[1]))
    desc = ProjectDesc() if desc is None else desc
    rgba = np.zeros((max(h, 0), max(w, 0), 4), np.float32)
    value = np.zeros((max(h, 0), max(w, 0)), np.float32)
    depth = np.zeros((max(h, 0), max(w, 0)), np.float32)
    _check(load().cvr_field_project_host(C.byref(f), C.byref(desc), _fp(iv), _fp(r2v), _fp(fr), w, h, int(offset[0]),
                                         int(offset[1]), rgba.ctypes.data, value.ctypes.data, depth.ctypes.data))
    return rgba, value, depth


def raw_transfer_table() -> np.ndarray:
    """The reference's Raw transfer table, (100, 4) floats (cvr_raw_transfer_table): the Raw scenes'
    albedo is classify_host(bytes, table, 0, max byte, ceil=True, density_u=True)."""
    out = np.empty((100, 4), np.float32)
    _check(load().cvr_raw_transfer_table(_fp(out)))
    return out


def _rotation9(rotation):
    """9 floats, row-major world-to-environment; None: zeros, which the library reads as identity."""
    if rotation is None:
        return np.zeros(9, np.float32)
    r = np.ascontiguousarray(rotation, dtype=np.float32).reshape(-1)
    if r.size != 9:
        raise ValueError(f"rotation: {r.size} floats, expected 9 (3 x 3, row-major)")
    return r


def rotation_y(degrees: float) -> np.ndarray:
    """The world-to-environment rotation that turns the map by `degrees` about +Y (the CLI's
    --env-rotate-y): (3, 3) float32, computed in fp64 and rounded once."""
    a = float(degrees) * (math.pi / 180.0)
    c, s = math.cos(a), math.sin(a)
    return np.array([[c, 0.0, -s], [0.0, 1.0, 0.0], [s, 0.0, c]], np.float64).astype(np.float32)


def _dirs3(dirs):
    d = np.ascontiguousarray(dirs, dtype=np.float32)
    if d.ndim != 2 or d.shape[1] != 3:
        raise ValueError(f"dirs: shape {d.shape}, expected (n, 3)")
    return d


def environment_eval_host(image, dirs, scale: float = 1.0, rotation=None) -> np.ndarray:
    """The environment lookup's written statement on the CPU (cvr_environment_eval_host; no GPU):
    image (H, W, 3|4) float32, row 0 the top; dirs (n, 3) -> (n, 3) radiance.
    Context.environment_eval and the render kernels compute the same bits."""
    img = np.ascontiguousarray(image, dtype=np.float32)
    if img.ndim != 3:
        raise ValueError(f"image: shape {img.shape}, expected (H, W, 3|4)")
    d = _dirs3(dirs)
    desc = EnvironmentDesc(img.shape[1], img.shape[0], img.shape[2], ENV_HOST, img.ctypes.data, scale)
    desc.rotation[:] = _rotation9(rotation).tolist()
    out = np.empty_like(d)
    _check(load().cvr_environment_eval_host(C.byref(desc), _fp(d), d.shape[0], _fp(out)))
    return out


def environment_eval_host_fn(width: int, height: int, texel, dirs, rotation=None) -> np.ndarray:
    """The same statement with the stored texels behind a callback, texel(x, y) -> (r, g, b), for
    maps too large to hold on the host (cvr_environment_eval_host_fn; no scale is applied)."""
    d = _dirs3(dirs)

    def cb(_user, x, y, rgba):
        v = texel(x, y)
        rgba[0], rgba[1], rgba[2] = float(v[0]), float(v[1]), float(v[2])

    r = None if rotation is None else _rotation9(rotation)
    out = np.empty_like(d)
    _check(load().cvr_environment_eval_host_fn(width, height, None if r is None else _fp(r), TEXEL_FN(cb), None,
                                               _fp(d), d.shape[0], _fp(out)))
    return out


def read_image(path: str) -> np.ndarray:
    """A Radiance .hdr or colour .pfm file as (H, W, 3) float32, row 0 the top (cvr_read_image)."""
    w, h = C.c_uint32(), C.c_uint32()
    p = C.POINTER(C.c_float)()
    _check(load().cvr_read_image(os.fsencode(path), C.byref(w), C.byref(h), C.byref(p)))
    try:
        return np.ctypeslib.as_array(p, shape=(h.value, w.value, 3)).copy()
    finally:
        load().cvr_free_image(p)


def _device_ptr(a):
    """An int address, or an object with data_ptr() (a torch tensor); None stays None."""
    if a is None:
        return None
    return int(a.data_ptr()) if hasattr(a, "data_ptr") else int(a)


def _check_device_grid(name, t, shape, device, dtypes=("float32",)):
    """ValueError unless the tensor-like `t` (an object with data_ptr()) is a contiguous array of
    `shape` and one of `dtypes` on cuda device `device`; attributes it does not have are not judged."""
    dtype = getattr(t, "dtype", None)
    if dtype is not None and str(dtype).split(".")[-1] not in dtypes:
        raise ValueError(f"{name}: dtype {dtype}, expected {' or '.join(dtypes)}")
    contiguous = getattr(t, "is_contiguous", None)
    if contiguous is not None and not contiguous():
        raise ValueError(f"{name}: not contiguous")
    if tuple(t.shape) != tuple(shape):
        raise ValueError(f"{name}: shape {tuple(t.shape)}, expected {tuple(shape)}")
    dev = getattr(t, "device", None)
    if dev is not None:
        kind, index = getattr(dev, "type", None), getattr(dev, "index", None)
        if kind != "cuda" or (index is not None and index != device):
            raise ValueError(f"{name}: on {dev}, the context is on cuda:{device}")


def default_camera(width: int, height: int):
    """Camera.h:25-71 + CudaVolPath.cpp:67-85 -> (inv_view[12], raster_to_view[2])."""
    lib = load()
    iv = np.zeros(12, np.float32)
    r2v = np.zeros(2, np.float32)
    _check(lib.cvr_default_camera(width, height, _fp(iv), _fp(r2v)))
    return iv, r2v


def tiling(width: int, height: int, ntx: int, nty: int):
    lib = load()
    td = (C.c_uint32 * 2)()
    _check(lib.cvr_tiling(width, height, ntx, nty, td))
    return int(td[0]), int(td[1])


def tile_origin(tile_id: int, ntx: int, tile_dim: Sequence[int]):
    lib = load()
    td = (C.c_uint32 * 2)(*tile_dim)
    org = (C.c_uint32 * 2)()
    _check(lib.cvr_tile_origin(tile_id, ntx, td, org))
    return int(org[0]), int(org[1])


def image_to_host(device_ptr: int, host_ptr: int, n_floats: int, scale: float, stream_ptr: Optional[int]):
    """host[i] = device[i] / scale, written by a kernel on `stream_ptr` into
    pinned or registered host memory (cvr_image_to_host; asynchronous)."""
    _check(load().cvr_image_to_host(C.c_void_p(device_ptr), C.c_void_p(host_ptr), n_floats, scale,
                                    C.c_void_p(stream_ptr) if stream_ptr else None))


def blocks_to_host(device_ptr: int, host_ptr: int, width: int, height: int, rank: int, world: int, scale: float,
                   stream_ptr: Optional[int]):
    """The pixels of block shard (rank, world) of a width x height float4
    image, divided by scale, stored by a kernel on `stream_ptr` at their places
    in the full pinned/registered host image (cvr_blocks_to_host; asynchronous)."""
    _check(load().cvr_blocks_to_host(C.c_void_p(device_ptr), C.c_void_p(host_ptr), width, height, rank, world,
                                     scale, C.c_void_p(stream_ptr) if stream_ptr else None))


def write_hdr(path: str, rgba: np.ndarray):
    rgba = np.ascontiguousarray(rgba, dtype=np.float32)
    h, w = rgba.shape[:2]
    _check(load().cvr_write_hdr(path.encode(), _fp(rgba), w, h))


# ------------------------------------------------------------------- scenes --
class Scene:
    """A loaded or synthetic scene (SceneBuilder + Scene, Scene.h:56-81)."""

    def __init__(self, handle):
        self._h = handle
        self.is_sparse = bool(load().cvr_scene_is_sparse(self._h))
        self._sparse = None
        self.medium = None
        if not self.is_sparse:
            self.medium = MediumDesc()
            _check(load().cvr_scene_medium(self._h, C.byref(self.medium)))

    @property
    def sparse_medium(self) -> SparseMediumDesc:
        """8^3-leaf view (cvr_scene_sparse_medium; built once for dense scenes)."""
        if self._sparse is None:
            d = SparseMediumDesc()
            _check(load().cvr_scene_sparse_medium(self._h, C.byref(d)))
            self._sparse = d
        return self._sparse

    @classmethod
    def synthetic(cls, name: str, seed: int = 0, dims: Optional[Sequence[int]] = None) -> "Scene":
        lib = load()
        h = C.c_void_p()
        d = (C.c_uint32 * 3)(*dims) if dims is not None else None
        _check(lib.cvr_scene_synthetic(name.encode(), seed, d, C.byref(h)))
        return cls(h)

    @classmethod
    def load(cls, path: str, scene_type: str = "Auto", default_albedo: Optional[Sequence[float]] = None) -> "Scene":
        """Load a scene file (cvr_scene_load_ex).  default_albedo (r, g, b): a VDB
        file without an albedo grid loads with that albedo everywhere (quirk
        Q17's flag; the reference refuses such files, VDBAdapter.cpp:32-37)."""
        lib = load()
        h = C.c_void_p()
        opts = None
        if default_albedo is not None:
            opts = LoadOptions()
            opts.flags = LOAD_DEFAULT_ALBEDO
            opts.default_albedo[:] = [float(v) for v in default_albedo]
        _check(lib.cvr_scene_load_ex(path.encode(), SCENE_TYPES[scene_type],
                                     C.byref(opts) if opts is not None else None, C.byref(h)))
        return cls(h)

    def camera(self, width: int, height: int):
        """(inv_view[12], raster_to_view[2]) of this scene's camera (cvr_scene_camera)."""
        iv = np.zeros(12, np.float32)
        r2v = np.zeros(2, np.float32)
        _check(load().cvr_scene_camera(self._h, width, height, _fp(iv), _fp(r2v)))
        return iv, r2v

    @property
    def dims(self):
        return tuple(int(v) for v in (self.sparse_medium if self.is_sparse else self.medium).res)

    def _dense_only(self):
        if self.is_sparse:
            raise CvrError(-5, "scene is stored sparse only (use leaves() / sparse_medium)")

    @property
    def max_density(self) -> float:
        return float((self.sparse_medium if self.is_sparse else self.medium).max_density)

    @property
    def has_albedo(self) -> bool:
        """Whether the medium stores albedo voxels (a sparse scene may use albedo_bg everywhere)."""
        return (not self.is_sparse) or bool(self.sparse_medium.leaf_albedo)

    def leaves(self):
        """(leaf_table (lz, ly, lx) u32, leaf_density (n, 8, 8, 8), leaf_albedo (n, 8, 8, 8, 4) or
        None, albedo_background) as numpy views owned by the scene."""
        d = self.sparse_medium
        lx, ly, lz = (int(v) for v in d.leaf_dims)
        table = np.ctypeslib.as_array(d.leaf_table, shape=(lz, ly, lx))
        n = int(d.n_leaves)
        dens = np.ctypeslib.as_array(d.leaf_density, shape=(n, 8, 8, 8)) if n else np.zeros((0, 8, 8, 8), np.float32)
        alb = np.ctypeslib.as_array(d.leaf_albedo, shape=(n, 8, 8, 8, 4)) if (n and d.leaf_albedo) else None
        return table, dens, alb, tuple(d.albedo_background)

    @property
    def density(self) -> np.ndarray:
        """(z, y, x) view of the fp32 density grid (owned by the scene)."""
        self._dense_only()
        nx, ny, nz = self.dims
        return np.ctypeslib.as_array(self.medium.density, shape=(nz, ny, nx))

    @property
    def albedo(self) -> np.ndarray:
        self._dense_only()
        nx, ny, nz = self.dims
        return np.ctypeslib.as_array(self.medium.albedo, shape=(nz, ny, nx, 4))

    @property
    def raw_bytes(self) -> bytes:
        p = C.POINTER(C.c_uint8)()
        n = C.c_size_t()
        _check(load().cvr_scene_raw_bytes(self._h, C.byref(p), C.byref(n)))
        return bytes(np.ctypeslib.as_array(p, shape=(n.value,))) if n.value else b""

    def close(self):
        if self._h:
            load().cvr_scene_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def medium_from_arrays(density: np.ndarray, albedo: np.ndarray, box_min=(-0.5,) * 3, box_max=(0.5,) * 3,
                       scale=100.0, max_density=None, g=0.0, roughness=(0.1, 0.1), eta=None):
    """Build a MediumDesc over caller arrays (kept alive by the returned tuple)."""
    density = np.ascontiguousarray(density, dtype=np.float32)
    albedo = np.ascontiguousarray(albedo, dtype=np.float32)
    nz, ny, nx = density.shape
    assert albedo.shape == (nz, ny, nx, 4)
    m = MediumDesc()
    m.res[:] = (nx, ny, nz)
    m.density = _fp(density)
    m.albedo = _fp(albedo)
    m.box_min[:] = box_min
    m.box_max[:] = box_max
    m.scale = scale
    m.max_density = float(density.max()) if max_density is None else max_density
    m.g = g
    m.roughness[:] = roughness
    m.eta = np.float32(np.float32(1.05) / np.float32(1.01)) if eta is None else eta
    return m, (density, albedo)


# ------------------------------------------------------------------ context --
class Context:
    """One kernel launcher bound to one GPU (VolPTKernelLauncher, RenderKernelLauncher.h:54-73)."""

    def __init__(self, device: int = 0, kernel="regenerationSK"):
        lib = load()
        kid = KERNELS.index(kernel) if isinstance(kernel, str) else int(kernel)
        h = C.c_void_p()
        _check(lib.cvr_create(device, kid, C.byref(h)))
        self._h = h
        self.kernel = kid
        self.device = device

    def _c(self, code):
        _check(code, self._h)

    def set_medium(self, medium: MediumDesc):
        self._c(load().cvr_set_medium(self._h, C.byref(medium)))

    def set_medium_sparse(self, desc: SparseMediumDesc):
        self._c(load().cvr_set_medium_sparse(self._h, C.byref(desc)))

    def set_medium_device(self, density, albedo=None, *, const_albedo=None, sparse=False, max_density=None,
                          res=None, box_min=(-0.5,) * 3, box_max=(0.5,) * 3, scale=100.0, g=0.0,
                          roughness=(0.1, 0.1), eta=None):
        """The medium from device memory, no host copy (cvr_set_medium_device): the state
        set_medium / set_medium_sparse leave on host copies of the same arrays.  density: (z, y, x)
        float32; albedo: (z, y, x, 4) float32, or None with const_albedo (4 floats: every voxel's
        albedo).  Each an object with data_ptr() (a torch tensor on the context's device,
        contiguous: checked here, ValueError) or an int device address (then res = (x, y, z) is
        required and nothing is checked here).  sparse: store as 8^3 leaves by the rule of cvr.h.
        max_density None: the largest density, found on the device.  Synchronous; torch's current
        stream is synchronised first, the tensors are only read and may be freed afterwards."""
        if (albedo is None) == (const_albedo is None):
            raise ValueError("set_medium_device: give exactly one of albedo and const_albedo")
        tensors = [t for t in (density, albedo) if hasattr(t, "data_ptr")]
        if res is None:
            if not hasattr(density, "data_ptr"):
                raise ValueError("set_medium_device: res is required with an int address")
            if len(density.shape) != 3:
                raise ValueError(f"density: shape {tuple(density.shape)}, expected (z, y, x)")
            nz, ny, nx = (int(v) for v in density.shape)
        else:
            nx, ny, nz = (int(v) for v in res)
        if hasattr(density, "data_ptr"):
            _check_device_grid("density", density, (nz, ny, nx), self.device)
        if hasattr(albedo, "data_ptr"):
            _check_device_grid("albedo", albedo, (nz, ny, nx, 4), self.device)
        if const_albedo is not None and len(const_albedo) != 4:
            raise ValueError("const_albedo: expected 4 floats")
        d = DeviceMediumDesc()
        d.res[:] = (nx, ny, nz)
        d.flags = ((DEVMED_SPARSE if sparse else 0) | (DEVMED_CONST_ALBEDO if albedo is None else 0)
                   | (DEVMED_MAX_DENSITY if max_density is None else 0))
        d.d_density = _device_ptr(density)
        d.d_albedo = _device_ptr(albedo)
        if const_albedo is not None:
            d.const_albedo[:] = [float(v) for v in const_albedo]
        d.box_min[:] = box_min
        d.box_max[:] = box_max
        d.scale = scale
        d.max_density = 0.0 if max_density is None else max_density
        d.g = g
        d.roughness[:] = roughness
        d.eta = np.float32(np.float32(1.05) / np.float32(1.01)) if eta is None else eta
        if any(type(t).__module__.split(".")[0] == "torch" for t in tensors):
            import torch
            torch.cuda.current_stream(self.device).synchronize()
        self._c(load().cvr_set_medium_device(self._h, C.byref(d)))

    def set_medium_scalar(self, scalar, table, *, lo, hi, ceil=False, density_u=False, sparse=False,
                          max_density=None, scalar_type=None, res=None, box_min=(-0.5,) * 3, box_max=(0.5,) * 3,
                          scale=100.0, g=0.0, roughness=(0.1, 0.1), eta=None):
        """The medium from a scalar field in device memory and a transfer table, classified inside
        the build kernels (cvr_set_medium_scalar): the state set_medium_device leaves on device
        copies of classify_host(scalar, table, lo, hi, ceil, density_u).  scalar: (z, y, x) uint8,
        int16, uint16 or float32, an object with data_ptr() (a torch tensor on the context's device,
        contiguous: checked here, ValueError) or an int device address (then scalar_type, a
        SCALAR_* value, and res = (x, y, z) are required and nothing is checked here).  table:
        (n, 4) floats (r, g, b, density) in host memory, n 2..4096.  The other arguments are
        set_medium_device's.  Synchronous; torch's current stream is synchronised first, the tensor
        is only read and may be freed afterwards; a new table means a new call."""
        is_tensor = hasattr(scalar, "data_ptr")
        if res is None:
            if not is_tensor:
                raise ValueError("set_medium_scalar: res is required with an int address")
            if len(scalar.shape) != 3:
                raise ValueError(f"scalar: shape {tuple(scalar.shape)}, expected (z, y, x)")
            nz, ny, nx = (int(v) for v in scalar.shape)
        else:
            nx, ny, nz = (int(v) for v in res)
        if is_tensor:
            _check_device_grid("scalar", scalar, (nz, ny, nx), self.device, tuple(_SCALAR_TYPES))
        if scalar_type is None:
            name = str(getattr(scalar, "dtype", "")).split(".")[-1]
            if name not in _SCALAR_TYPES:
                raise ValueError("set_medium_scalar: scalar_type is required with an int address")
            scalar_type = _SCALAR_TYPES[name]
        t, _tab = _transfer_desc(table, lo, hi, ceil, density_u)
        d = ScalarMediumDesc()
        d.res[:] = (nx, ny, nz)
        d.flags = (DEVMED_SPARSE if sparse else 0) | (DEVMED_MAX_DENSITY if max_density is None else 0)
        d.d_scalar = _device_ptr(scalar)
        d.scalar_type = scalar_type
        d.transfer = t
        d.box_min[:] = box_min
        d.box_max[:] = box_max
        d.scale = scale
        d.max_density = 0.0 if max_density is None else max_density
        d.g = g
        d.roughness[:] = roughness
        d.eta = np.float32(np.float32(1.05) / np.float32(1.01)) if eta is None else eta
        if is_tensor and type(scalar).__module__.split(".")[0] == "torch":
            import torch
            torch.cuda.current_stream(self.device).synchronize()
        self._c(load().cvr_set_medium_scalar(self._h, C.byref(d)))

    def set_medium_gradient(self, scalar, table, *, lo, hi, glo, ghi, spacing=(1.0, 1.0, 1.0), sparse=False,
                            max_density=None, scalar_type=None, res=None, box_min=(-0.5,) * 3, box_max=(0.5,) * 3,
                            scale=100.0, g=0.0, roughness=(0.1, 0.1), eta=None):
        """The medium from a scalar field in device memory and a 2-D transfer table over the value
        and the gradient magnitude, classified inside the build kernels (cvr_set_medium_gradient):
        the state set_medium_device leaves on device copies of classify_gradient_host(scalar,
        table, lo, hi, glo, ghi, spacing)'s density and albedo.  table: (m, n, 4) floats in host
        memory, n >= 2, m >= 2, n * m <= 4096.  scalar and the other arguments are
        set_medium_scalar's.  Synchronous; torch's current stream is synchronised first, the tensor
        is only read and may be freed afterwards; a new table means a new call."""
        is_tensor = hasattr(scalar, "data_ptr")
        if res is None:
            if not is_tensor:
                raise ValueError("set_medium_gradient: res is required with an int address")
            if len(scalar.shape) != 3:
                raise ValueError(f"scalar: shape {tuple(scalar.shape)}, expected (z, y, x)")
            nz, ny, nx = (int(v) for v in scalar.shape)
        else:
            nx, ny, nz = (int(v) for v in res)
        if is_tensor:
            _check_device_grid("scalar", scalar, (nz, ny, nx), self.device, tuple(_SCALAR_TYPES))
        if scalar_type is None:
            name = str(getattr(scalar, "dtype", "")).split(".")[-1]
            if name not in _SCALAR_TYPES:
                raise ValueError("set_medium_gradient: scalar_type is required with an int address")
            scalar_type = _SCALAR_TYPES[name]
        t, _tab = _gradient_transfer_desc(table, lo, hi, glo, ghi, spacing)
        d = GradientMediumDesc()
        d.res[:] = (nx, ny, nz)
        d.flags = (DEVMED_SPARSE if sparse else 0) | (DEVMED_MAX_DENSITY if max_density is None else 0)
        d.d_scalar = _device_ptr(scalar)
        d.scalar_type = scalar_type
        d.transfer = t
        d.box_min[:] = box_min
        d.box_max[:] = box_max
        d.scale = scale
        d.max_density = 0.0 if max_density is None else max_density
        d.g = g
        d.roughness[:] = roughness
        d.eta = np.float32(np.float32(1.05) / np.float32(1.01)) if eta is None else eta
        if is_tensor and type(scalar).__module__.split(".")[0] == "torch":
            import torch
            torch.cuda.current_stream(self.device).synchronize()
        self._c(load().cvr_set_medium_gradient(self._h, C.byref(d)))

    def set_medium_labeled(self, scalar, labels, table, *, lo, hi, ceil=False, density_u=False, sparse=False,
                           max_density=None, scalar_type=None, res=None, box_min=(-0.5,) * 3, box_max=(0.5,) * 3,
                           scale=100.0, g=0.0, roughness=(0.1, 0.1), eta=None):
        """The medium from a scalar field and a label volume in device memory and a table of one
        transfer function per label, classified inside the build kernels (cvr_set_medium_labeled):
        the state set_medium_device leaves on device copies of classify_labels_host(scalar, labels,
        table, lo, hi, ceil, density_u)'s density and albedo.  table: (m, n, 4) floats in host
        memory, n >= 2, 1 <= m <= 256, n * m <= 4096; a label byte >= m takes row 0.  labels: a
        uint8 tensor (contiguous, on the context's device, as many elements as scalar: checked
        here, ValueError), or anything with data_ptr(), or an int device address, of any alignment.
        scalar and the other arguments are set_medium_scalar's; views at an offset are fine for
        both.  Synchronous; torch's current stream is synchronised first, both tensors are only
        read and may be freed afterwards; a new table means a new call."""
        is_tensor = hasattr(scalar, "data_ptr")
        if res is None:
            if not is_tensor:
                raise ValueError("set_medium_labeled: res is required with an int address")
            if len(scalar.shape) != 3:
                raise ValueError(f"scalar: shape {tuple(scalar.shape)}, expected (z, y, x)")
            nz, ny, nx = (int(v) for v in scalar.shape)
        else:
            nx, ny, nz = (int(v) for v in res)
        if is_tensor:
            _check_device_grid("scalar", scalar, (nz, ny, nx), self.device, tuple(_SCALAR_TYPES))
        if scalar_type is None:
            name = str(getattr(scalar, "dtype", "")).split(".")[-1]
            if name not in _SCALAR_TYPES:
                raise ValueError("set_medium_labeled: scalar_type is required with an int address")
            scalar_type = _SCALAR_TYPES[name]
        if hasattr(labels, "data_ptr") and hasattr(labels, "shape"):
            count = 1
            for v in labels.shape:
                count *= int(v)
            if count != nx * ny * nz:
                raise ValueError(f"labels: {count} elements, the field has {nx * ny * nz}")
            _check_device_grid("labels", labels, tuple(labels.shape), self.device, ("uint8",))
        t, _tab = _label_transfer_desc(table, lo, hi, ceil, density_u)
        d = LabeledMediumDesc()
        d.res[:] = (nx, ny, nz)
        d.flags = (DEVMED_SPARSE if sparse else 0) | (DEVMED_MAX_DENSITY if max_density is None else 0)
        d.d_scalar = _device_ptr(scalar)
        d.d_labels = _device_ptr(labels)
        d.scalar_type = scalar_type
        d.transfer = t
        d.box_min[:] = box_min
        d.box_max[:] = box_max
        d.scale = scale
        d.max_density = 0.0 if max_density is None else max_density
        d.g = g
        d.roughness[:] = roughness
        d.eta = np.float32(np.float32(1.05) / np.float32(1.01)) if eta is None else eta
        if any(type(v).__module__.split(".")[0] == "torch" for v in (scalar, labels)):
            import torch
            torch.cuda.current_stream(self.device).synchronize()
        self._c(load().cvr_set_medium_labeled(self._h, C.byref(d)))

    def medium_label_info(self):
        """(m, counts) of the medium in use, own or shared (cvr_medium_label_info): the rows of the
        table set_medium_labeled built it with (0: another call built it) and 256 uint64, the
        voxels per label byte that the build kept (a clip's voxels are not counted, so they sum to
        medium_clip_info()'s kept), counted on the device during the build."""
        m = C.c_uint32(0)
        counts = np.zeros(256, np.uint64)
        self._c(load().cvr_medium_label_info(self._h, C.byref(m), counts.ctypes.data_as(C.POINTER(C.c_uint64))))
        return int(m.value), counts

    def set_clip(self, lo=None, hi=None, planes=()):
        """The clip region of the next device builds (cvr_set_clip): a crop box lo <= c < hi in
        (x, y, z) voxel indices (None: no bound; hi past the grid means "to the end") and up to 8
        planes (A, B, C, D) in voxel-index space (plane_from_box makes one from box coordinates).
        set_medium_device, set_medium_scalar and set_medium_gradient then store a voxel outside
        the region as empty (density 0, voxel 0's albedo): clip_host is the statement.  The
        medium already built is not touched; the host uploads refuse while a clip is set."""
        d = _clip_desc(lo, hi, planes)
        self._c(load().cvr_set_clip(self._h, C.byref(d)))

    def clear_clip(self):
        self._c(load().cvr_clear_clip(self._h))

    @property
    def clip(self):
        """The clip set on the context as {"lo", "hi", "planes"}, or None."""
        d, on = ClipDesc(), C.c_int(0)
        self._c(load().cvr_get_clip(self._h, C.byref(d), C.byref(on)))
        return d.as_dict() if on.value else None

    def medium_clip_info(self):
        """(the clip the medium in use was built under as {"lo", "hi", "planes"}, the number of
        voxels it keeps, counted on the device during the build); a medium built without a clip:
        the region that keeps everything and the grid's voxel count."""
        d, kept = ClipDesc(), C.c_uint64(0)
        self._c(load().cvr_medium_clip_info(self._h, C.byref(d), C.byref(kept)))
        return d.as_dict(), int(kept.value)

    def _device_field(self, what, scalar, spacing, scalar_type, res):
        """(FieldDesc, is a torch tensor) of what set_medium_gradient accepts as `scalar`, with its checks."""
        is_tensor = hasattr(scalar, "data_ptr")
        if res is None:
            if not is_tensor:
                raise ValueError(f"{what}: res is required with an int address")
            if len(scalar.shape) != 3:
                raise ValueError(f"scalar: shape {tuple(scalar.shape)}, expected (z, y, x)")
            nz, ny, nx = (int(v) for v in scalar.shape)
        else:
            nx, ny, nz = (int(v) for v in res)
        if is_tensor:
            _check_device_grid("scalar", scalar, (nz, ny, nx), self.device, tuple(_SCALAR_TYPES))
        if scalar_type is None:
            name = str(getattr(scalar, "dtype", "")).split(".")[-1]
            if name not in _SCALAR_TYPES:
                raise ValueError(f"{what}: scalar_type is required with an int address")
            scalar_type = _SCALAR_TYPES[name]
        f = _field_desc(_device_ptr(scalar), scalar_type, (nx, ny, nz), spacing)
        return f, is_tensor and type(scalar).__module__.split(".")[0] == "torch"

    def field_stats(self, scalar, spacing=(1.0, 1.0, 1.0), scalar_type=None, res=None) -> "FieldStats":
        """field_stats_host of a scalar field in device memory (cvr_field_stats), the same bits:
        the lo, hi and ghi a transfer table can be aimed with.  scalar is what set_medium_gradient
        accepts.  Synchronous; torch's current stream is synchronised first; the context's medium
        and framebuffer are not touched."""
        f, torch_tensor = self._device_field("field_stats", scalar, spacing, scalar_type, res)
        if torch_tensor:
            import torch
            torch.cuda.current_stream(self.device).synchronize()
        st = FieldStatsStruct()
        self._c(load().cvr_field_stats(self._h, C.byref(f), C.byref(st)))
        return _field_stats(st)

    def field_histogram(self, scalar, n, m=1, *, lo, hi, glo=None, ghi=None, spacing=(1.0, 1.0, 1.0), out=None,
                        scalar_type=None, res=None):
        """field_histogram_host of a scalar field in device memory (cvr_field_histogram), the same
        counts, as an (m, n) numpy uint32 array.  With out= a device tensor or address of n * m
        32-bit words the counts are written there (cvr_field_histogram_buffers: ordered on the
        context's stream, not synchronised, every word overwritten) and `out` is returned.  scalar
        is what set_medium_gradient accepts; torch's current stream is synchronised first."""
        f, torch_tensor = self._device_field("field_histogram", scalar, spacing, scalar_type, res)
        h = _histogram_desc(n, m, lo, hi, glo, ghi)
        if out is not None and hasattr(out, "data_ptr"):
            size = getattr(out, "element_size", lambda: 4)()
            numel = getattr(out, "numel", lambda: int(n) * int(m))()
            if size != 4 or numel != int(n) * int(m):
                raise ValueError(f"out: {numel} elements of {size} bytes, expected {int(n) * int(m)} 32-bit words")
            contiguous = getattr(out, "is_contiguous", None)
            if contiguous is not None and not contiguous():
                raise ValueError("out: not contiguous")
        if torch_tensor:
            import torch
            torch.cuda.current_stream(self.device).synchronize()
        if out is not None:
            self._c(load().cvr_field_histogram_buffers(self._h, C.byref(f), C.byref(h), _device_ptr(out)))
            return out
        counts = np.empty((max(int(m), 0), max(int(n), 0)), np.uint32)
        self._c(load().cvr_field_histogram(self._h, C.byref(f), C.byref(h), counts.ctypes.data))
        return counts

    def field_project(self, scalar, desc: Optional[ProjectDesc] = None, value=True, depth=True, scalar_type=None,
                      res=None):
        """field_project_host of a scalar field in device memory (cvr_field_project) for the
        context's camera, resolution and offset, the same bits: (rgba (h, w, 4), value (h, w),
        depth (h, w)) as numpy arrays; value / depth False: that plane is not computed and None is
        returned for it.  scalar is what set_medium_gradient accepts.  Synchronous; torch's current
        stream is synchronised first; the context needs no medium and is only read."""
        f, torch_tensor = self._device_field("field_project", scalar, (1.0, 1.0, 1.0), scalar_type, res)
        desc = ProjectDesc() if desc is None else desc
        if torch_tensor:
            import torch
            torch.cuda.current_stream(self.device).synchronize()
        w, h = self.resolution
        rgba = np.zeros((h, w, 4), np.float32)
        v = np.zeros((h, w), np.float32) if value else None
        z = np.zeros((h, w), np.float32) if depth else None
        self._c(load().cvr_field_project(self._h, C.byref(f), C.byref(desc), rgba.ctypes.data,
                                         None if v is None else v.ctypes.data, None if z is None else z.ctypes.data,
                                         rgba.size))
        return rgba, v, z

    def field_project_buffers(self, scalar, out_rgba, out_value=None, out_depth=None, desc: Optional[ProjectDesc] = None,
                              scalar_type=None, res=None):
        """The projection into device buffers (cvr_field_project_buffers), ordered on the context's
        stream and not synchronised (the field must stay until it has run): out_rgba tile_w * tile_h
        * 4 floats (16-byte aligned), out_value and out_depth tile_w * tile_h floats or None; each an
        int device address or an object with data_ptr() (a torch tensor).  torch's current stream is
        synchronised first."""
        f, torch_tensor = self._device_field("field_project_buffers", scalar, (1.0, 1.0, 1.0), scalar_type, res)
        desc = ProjectDesc() if desc is None else desc
        if torch_tensor:
            import torch
            torch.cuda.current_stream(self.device).synchronize()
        self._c(load().cvr_field_project_buffers(self._h, C.byref(f), C.byref(desc), _device_ptr(out_rgba),
                                                 _device_ptr(out_value), _device_ptr(out_depth)))

    def set_environment(self, image, scale: float = 1.0, rotation=None):
        """Light the scene with a latitude-longitude map (cvr_set_environment): an escaping path adds
        its throughput times the map's radiance in its direction.  image: a numpy (H, W, 3|4)
        float32 array (row 0 the top), or an object with data_ptr() of that shape (a torch tensor on
        the context's device, contiguous: checked here, ValueError), which is converted on the
        device with no host copy.  scale multiplies every component; rotation: 9 floats, row-major
        world-to-environment (None: identity).  The context keeps its own copy."""
        d = EnvironmentDesc()
        if hasattr(image, "data_ptr"):
            shape = tuple(int(v) for v in image.shape)
            if len(shape) != 3:
                raise ValueError(f"image: shape {shape}, expected (H, W, 3|4)")
            _check_device_grid("image", image, shape, self.device)
            keep, d.location, d.pixels = image, ENV_DEVICE, _device_ptr(image)
            if type(image).__module__.split(".")[0] == "torch":
                import torch
                torch.cuda.current_stream(self.device).synchronize()
        else:
            keep = np.ascontiguousarray(image, dtype=np.float32)
            shape = keep.shape
            if keep.ndim != 3:
                raise ValueError(f"image: shape {shape}, expected (H, W, 3|4)")
            d.location, d.pixels = ENV_HOST, keep.ctypes.data
        d.height, d.width, d.channels = shape
        d.scale = scale
        d.rotation[:] = _rotation9(rotation).tolist()
        self._c(load().cvr_set_environment(self._h, C.byref(d)))
        del keep

    def clear_environment(self):
        """Back to the constant environment of radiance 1 (cvr_clear_environment)."""
        self._c(load().cvr_clear_environment(self._h))

    def environment_info(self) -> EnvironmentInfo:
        """The stored map's width, height, device bytes and largest component (0 x 0: none)."""
        out = EnvironmentInfo()
        self._c(load().cvr_environment_info(self._h, C.byref(out)))
        return out

    def environment_eval(self, dirs) -> np.ndarray:
        """The device's lookup of the context's environment for dirs (n, 3) -> (n, 3)
        (cvr_environment_eval): the same bits as environment_eval_host."""
        d = _dirs3(dirs)
        out = np.empty_like(d)
        self._c(load().cvr_environment_eval(self._h, _fp(d), d.shape[0], _fp(out)))
        return out

    def trace_env(self, first: int, count: int) -> np.ndarray:
        """trace_paths' walk with the environment applied (cvr_trace_env): records of image_id, flags,
        n_segments, T (before the environment), d (at escape) and C = T * L(d)."""
        out = np.zeros(count, ENV_RECORD_DTYPE)
        self._c(load().cvr_trace_env(self._h, first, count, out.ctypes.data_as(C.POINTER(EnvRecord))))
        return out

    def medium_layout(self) -> MediumLayout:
        """What the upload built (cvr_medium_layout): sparse or dense, uniform albedo and its value,
        leaves, cell leaves, brick and mask shifts and the empty-region mask's 64 words."""
        ml = MediumLayout()
        self._c(load().cvr_medium_layout(self._h, C.byref(ml)))
        return ml

    def device_medium_ms(self):
        """Device ms of the last set_medium_device, set_medium_scalar or set_medium_gradient by group, with OPT_TIMING 1
        (cvr_debug_device_medium_ms): density scan, albedo scan, leaf flags, scans and scatters,
        copy / gather, cells + bounds + brick words."""
        out = (C.c_double * 6)()
        self._c(load().cvr_debug_device_medium_ms(self._h, out))
        return list(out)

    def debug_medium_array(self, which):
        """One stored array of the medium in use, as stored (cvr_debug_copy_medium).  which: a
        MEDIUM_* value or its lower-case name ("density", "leaf_table", ...).  Returns a flat numpy
        array of the natural dtype: float32 or float16 by the medium's format for values, uint32
        for tables, words and the mask, uint8 for the dense bounds; None when the medium has no
        such array."""
        if isinstance(which, str):
            which = MEDIUM_ARRAYS.index(which)
        lib = load()
        need = C.c_size_t(0)
        code = lib.cvr_debug_copy_medium(self._h, which, None, 0, C.byref(need))
        if need.value == 0:
            self._c(code)
            return None
        if MEDIUM_ARRAYS[which] in _MEDIUM_VALUE_ARRAYS:
            dtype = np.float16 if self.medium_info().format else np.float32
        else:
            dtype = np.uint8 if which == MEDIUM_BOUNDS else np.uint32
        out = np.empty(need.value // np.dtype(dtype).itemsize, dtype)
        self._c(lib.cvr_debug_copy_medium(self._h, which, out.ctypes.data, out.nbytes, C.byref(need)))
        return out

    def set_camera(self, inv_view, raster_to_view, full_res):
        iv = np.ascontiguousarray(inv_view, np.float32)
        r = np.ascontiguousarray(raster_to_view, np.float32)
        fr = np.ascontiguousarray(full_res, np.float32)
        self._c(load().cvr_set_camera(self._h, _fp(iv), _fp(r), _fp(fr)))

    def set_resolution(self, w, h):
        self._c(load().cvr_set_resolution(self._h, w, h))

    @property
    def resolution(self):
        """The tile resolution the library renders now (cvr_get_resolution): render_image /
        render_tiles set it to their tile size too."""
        w, h = C.c_uint32(), C.c_uint32()
        self._c(load().cvr_get_resolution(self._h, C.byref(w), C.byref(h)))
        return w.value, h.value

    def set_offset(self, x, y):
        self._c(load().cvr_set_offset(self._h, x, y))

    def set_iterations(self, it):
        self._c(load().cvr_set_iterations(self._h, it))

    def set_path_range(self, first, count):
        self._c(load().cvr_set_path_range(self._h, first, count))

    def set_block_shard(self, rank, world):
        """Launch only shard `rank` of `world` (cvr_set_block_shard)."""
        self._c(load().cvr_set_block_shard(self._h, rank, world))

    def share_medium(self, src: "Context"):
        """Render `src`'s medium without a copy (cvr_share_medium); keep `src` alive."""
        self._c(load().cvr_share_medium(self._h, src._h))
        self._medium_src = src

    def medium_info(self) -> MediumInfo:
        """Format, majorant in use and device bytes of the medium (a shared medium: the source's)."""
        mi = MediumInfo()
        self._c(load().cvr_medium_info(self._h, C.byref(mi)))
        return mi

    def set_block_order(self, perm: Optional[np.ndarray]):
        """Block work order of the launch (cvr_set_block_order); None = natural."""
        if perm is None:
            self._c(load().cvr_set_block_order(self._h, None, 0))
            return
        p = np.ascontiguousarray(perm, np.uint32)
        self._c(load().cvr_set_block_order(self._h, p.ctypes.data_as(C.c_void_p), len(p)))

    def launch_blocks(self):
        """(n_blocks, n_queues, qbeg) of the current launch's pixel-block work order."""
        nb, nq = C.c_uint32(), C.c_uint32()
        qb = (C.c_uint32 * 9)()
        self._c(load().cvr_launch_blocks(self._h, C.byref(nb), C.byref(nq), qb))
        return nb.value, nq.value, list(qb)[:nq.value + 1]

    def set_seed(self, seed):
        self._c(load().cvr_set_seed(self._h, seed))

    def get_seed(self) -> int:
        v = C.c_uint32()
        self._c(load().cvr_get_seed(self._h, C.byref(v)))
        return v.value

    def set_output(self, device_ptr: Optional[int]):
        self._c(load().cvr_set_output(self._h, C.c_void_p(device_ptr) if device_ptr else None))

    def output_ptr(self) -> int:
        return load().cvr_output_ptr(self._h) or 0

    def set_stream(self, stream_ptr: Optional[int]):
        """Launch on `stream_ptr` (a hipStream_t; 0/None = the null stream).  A different stream
        than the one in use: waits first for the work pending on the stream being left; the stream
        must stay valid until the context has left it or is closed (cvr_set_stream)."""
        self._c(load().cvr_set_stream(self._h, C.c_void_p(stream_ptr) if stream_ptr else None))

    def use_own_stream(self):
        self._c(load().cvr_set_stream(self._h, load().cvr_own_stream(self._h)))

    def set_option(self, opt: int, value: int):
        self._c(load().cvr_set_option(self._h, opt, value))

    def init(self):
        self._c(load().cvr_init(self._h))

    def launch_render(self):
        self._c(load().cvr_launch_render(self._h))

    def reset(self):
        self._c(load().cvr_reset(self._h))

    def synchronize(self):
        self._c(load().cvr_synchronize(self._h))

    def clear_output(self):
        self._c(load().cvr_clear_output(self._h))

    def stats(self) -> Stats:
        s = Stats()
        self._c(load().cvr_get_stats(self._h, C.byref(s)))
        return s

    def copy_output(self, w, h, scale=1.0) -> np.ndarray:
        out = np.zeros((h, w, 4), np.float32)
        self._c(load().cvr_copy_output(self._h, _fp(out), scale))
        return out

    def copy_moments(self):
        """(sum, m2): the raw framebuffer sums and the second moments (sum T^2 per channel, w: the
        pixel's escape count) of an OPT_MOMENTS 1 context, (h, w, 4) each (cvr_copy_moments)."""
        w, h = self.resolution
        s1 = np.zeros((h, w, 4), np.float32)
        s2 = np.zeros((h, w, 4), np.float32)
        self._c(load().cvr_copy_moments(self._h, _fp(s1), _fp(s2)))
        return s1, s2

    def denoise(self, desc: Optional[DenoiseDesc] = None, n_samples: Optional[int] = None, host_ptr=None) -> np.ndarray:
        """The context's framebuffer filtered with its second moments (cvr_denoise; OPT_MOMENTS 1):
        n_samples (>= 2) is the number of samples accumulated since the last clear; inside an
        adaptive session it stays None and every block has its own count.  Synchronous; the
        buffers are only read.  host_ptr: a PinnedImage to store into (returned as its array)."""
        desc = DenoiseDesc() if desc is None else desc
        if isinstance(host_ptr, PinnedImage):
            self._c(load().cvr_denoise(self._h, C.byref(desc), n_samples or 0, host_ptr.ptr, host_ptr.floats))
            return host_ptr.array
        w, h = self.resolution
        img = np.zeros((h, w, 4), np.float32)
        self._c(load().cvr_denoise(self._h, C.byref(desc), n_samples or 0, C.c_void_p(img.ctypes.data), img.size))
        return img

    def denoise_buffers(self, sum_rgba, m2_rgba, width: int, height: int, out_rgba, n_samples: Optional[int] = None,
                        block_samples=None, desc: Optional[DenoiseDesc] = None, out_var=None):
        """The denoiser on device buffers of any origin (cvr_denoise_buffers), asynchronous on the
        context's stream: each buffer an int device address or an object with data_ptr() (a torch
        tensor).  sum_rgba / m2_rgba / out_rgba: width * height * 4 floats, 16-byte aligned;
        block_samples: (height / 8) * (width / 8) uint32 on the device, or None with n_samples;
        out_var: width * height floats or None."""
        desc = DenoiseDesc() if desc is None else desc
        self._c(load().cvr_denoise_buffers(self._h, _device_ptr(sum_rgba), _device_ptr(m2_rgba), width, height,
                                           n_samples or 0, _device_ptr(block_samples), C.byref(desc),
                                           _device_ptr(out_rgba), _device_ptr(out_var)))

    def features(self, desc: Optional[FeaturesDesc] = None):
        """The feature pass on the context's medium, camera, resolution and offset (cvr_features):
        (feat_rgba (h, w, 4), feat_depth (h, w)), the bits of features_host.  Synchronous; the
        context is only read.  Available inside an adaptive session."""
        desc = FeaturesDesc() if desc is None else desc
        w, h = self.resolution
        rgba = np.zeros((h, w, 4), np.float32)
        depth = np.zeros((h, w), np.float32)
        self._c(load().cvr_features(self._h, C.byref(desc), C.c_void_p(rgba.ctypes.data), C.c_void_p(depth.ctypes.data),
                                    rgba.size))
        return rgba, depth

    def features_buffers(self, out_rgba, out_depth=None, desc: Optional[FeaturesDesc] = None):
        """The feature pass into device buffers (cvr_features_buffers), asynchronous on the context's
        stream: out_rgba tile_w * tile_h * 4 floats (16-byte aligned), out_depth tile_w * tile_h
        floats or None; each an int device address or an object with data_ptr() (a torch tensor)."""
        desc = FeaturesDesc() if desc is None else desc
        self._c(load().cvr_features_buffers(self._h, C.byref(desc), _device_ptr(out_rgba), _device_ptr(out_depth)))

    def preview(self, desc: Optional[PreviewDesc] = None, host_ptr=None) -> np.ndarray:
        """The shaded preview of the context's medium, camera, resolution and offset (cvr_preview):
        rgba (h, w, 4), the bits of preview_host.  Synchronous; the context is only read.  Available
        inside an adaptive session.  host_ptr: a PinnedImage the kernel stores into (returned as its
        array), or None for a new numpy array."""
        desc = PreviewDesc() if desc is None else desc
        w, h = self.resolution
        if isinstance(host_ptr, PinnedImage):
            self._c(load().cvr_preview(self._h, C.byref(desc), host_ptr.ptr, host_ptr.floats))
            return host_ptr.array
        rgba = np.zeros((h, w, 4), np.float32)
        self._c(load().cvr_preview(self._h, C.byref(desc), C.c_void_p(rgba.ctypes.data), rgba.size))
        return rgba

    def preview_buffers(self, out_rgba, desc: Optional[PreviewDesc] = None):
        """The shaded preview into a device buffer (cvr_preview_buffers), asynchronous on the
        context's stream: out_rgba tile_w * tile_h * 4 floats (16-byte aligned), an int device
        address or an object with data_ptr() (a torch tensor)."""
        desc = PreviewDesc() if desc is None else desc
        self._c(load().cvr_preview_buffers(self._h, C.byref(desc), _device_ptr(out_rgba)))

    def build_light_volume(self, light, res=None, march: Optional[FeaturesDesc] = None) -> LightVolumeDesc:
        """The light volume of the context's medium for the direction `light` towards the light
        (cvr_build_light_volume), asynchronous on the context's stream, into memory the context
        owns; it replaces the previous one.  res (x, y, z): None for min(256, ceil(medium res / 2))
        per axis.  Returns the descriptor used.  Available inside an adaptive session."""
        if res is None:
            r = (C.c_uint32 * 3)()
            self._c(load().cvr_light_volume_default_res(self._h, r))
            res = tuple(r)
        desc = LightVolumeDesc(res, light, march)
        self._c(load().cvr_build_light_volume(self._h, C.byref(desc)))
        return desc

    def light_volume_info(self) -> LightVolumeInfo:
        """res, the normalised light, bytes and `valid` of the context's light volume."""
        info = LightVolumeInfo()
        self._c(load().cvr_light_volume_info(self._h, C.byref(info)))
        return info

    def light_volume(self) -> np.ndarray:
        """The context's light volume (cvr_copy_light_volume): transmittances (z, y, x), the bits of
        light_volume_host.  Synchronous."""
        info = self.light_volume_info()
        out = np.zeros(tuple(info.res)[::-1] if info.valid else (0, 0, 0), np.float32)
        self._c(load().cvr_copy_light_volume(self._h, C.c_void_p(out.ctypes.data), out.size))
        return out

    def clear_light_volume(self):
        self._c(load().cvr_clear_light_volume(self._h))

    def preview_shadowed(self, desc: Optional[PreviewDesc] = None, shadow: float = 0.7, host_ptr=None) -> np.ndarray:
        """Context.preview with the context's light volume (cvr_preview_shadowed): every
        contributing sample's light scaled by 1 - shadow (1 - S), S the volume's value there; the
        bits of preview_shadowed_host.  desc None: the default shading without the headlight; its
        light is not read (the volume's is)."""
        desc = PreviewDesc(flags=0) if desc is None else desc
        w, h = self.resolution
        if isinstance(host_ptr, PinnedImage):
            self._c(load().cvr_preview_shadowed(self._h, C.byref(desc), float(shadow), host_ptr.ptr, host_ptr.floats))
            return host_ptr.array
        rgba = np.zeros((h, w, 4), np.float32)
        self._c(load().cvr_preview_shadowed(self._h, C.byref(desc), float(shadow), C.c_void_p(rgba.ctypes.data), rgba.size))
        return rgba

    def preview_shadowed_buffers(self, out_rgba, desc: Optional[PreviewDesc] = None, shadow: float = 0.7):
        """The shadowed preview into a device buffer (cvr_preview_shadowed_buffers), asynchronous on
        the context's stream; out_rgba as preview_buffers'."""
        desc = PreviewDesc(flags=0) if desc is None else desc
        self._c(load().cvr_preview_shadowed_buffers(self._h, C.byref(desc), float(shadow), _device_ptr(out_rgba)))

    def denoise_guided(self, desc: Optional[DenoiseGuidedDesc] = None, n_samples: Optional[int] = None,
                       features: Optional[FeaturesDesc] = None, host_ptr=None) -> np.ndarray:
        """Context.denoise with the feature guide (cvr_denoise_guided): the feature pass runs into
        planes the context owns, then the guided filter on the framebuffer and its moments."""
        desc = DenoiseGuidedDesc() if desc is None else desc
        features = FeaturesDesc() if features is None else features
        if isinstance(host_ptr, PinnedImage):
            self._c(load().cvr_denoise_guided(self._h, C.byref(desc), C.byref(features), n_samples or 0, host_ptr.ptr,
                                              host_ptr.floats))
            return host_ptr.array
        w, h = self.resolution
        img = np.zeros((h, w, 4), np.float32)
        self._c(load().cvr_denoise_guided(self._h, C.byref(desc), C.byref(features), n_samples or 0,
                                          C.c_void_p(img.ctypes.data), img.size))
        return img

    def denoise_guided_buffers(self, sum_rgba, m2_rgba, feat_rgba, feat_depth, width: int, height: int, out_rgba,
                               n_samples: Optional[int] = None, block_samples=None,
                               desc: Optional[DenoiseGuidedDesc] = None, out_var=None):
        """Context.denoise_buffers with two device feature planes of any origin
        (cvr_denoise_guided_buffers): feat_rgba width * height * 4 floats (16-byte aligned),
        feat_depth width * height floats."""
        desc = DenoiseGuidedDesc() if desc is None else desc
        self._c(load().cvr_denoise_guided_buffers(self._h, _device_ptr(sum_rgba), _device_ptr(m2_rgba), width, height,
                                                  n_samples or 0, _device_ptr(block_samples), C.byref(desc),
                                                  _device_ptr(feat_rgba), _device_ptr(feat_depth),
                                                  _device_ptr(out_rgba), _device_ptr(out_var)))

    def adaptive(self, desc: AdaptiveDesc) -> "AdaptiveSession":
        """A noise-targeted render of the set tile as a context manager (cvr_adaptive_begin ..
        cvr_adaptive_end): `with ctx.adaptive(desc) as a: while not a.step().done: ...; img = a.image()`."""
        return AdaptiveSession(self, desc)

    def render_adaptive(self, desc: AdaptiveDesc, host_ptr=None):
        """cvr_render_adaptive: passes until every 8x8 block meets desc.target or has
        desc.max_iterations samples.  Returns (image, AdaptiveResult, block error map, block
        samples map); the maps are (tile_h / 8, tile_w / 8), the summed counters are left in
        self.adaptive_stats.  host_ptr: a PinnedImage to store into (the image returned is then
        its array)."""
        w, h = self.resolution
        res, st = AdaptiveResult(), Stats()
        if isinstance(host_ptr, PinnedImage):
            img, ptr, n = host_ptr.array, host_ptr.ptr, host_ptr.floats
        else:
            img = np.zeros((h, w, 4), np.float32)
            ptr, n = C.c_void_p(img.ctypes.data), img.size
        self._c(load().cvr_render_adaptive(self._h, C.byref(desc), ptr, n, C.byref(res), C.byref(st)))
        self.adaptive_stats = st
        err, smp = _adaptive_maps(self)
        return img, res, err, smp

    def trace_paths(self, first: int, count: int) -> np.ndarray:
        out = np.zeros(count, PATH_RECORD_DTYPE)
        self._c(load().cvr_trace_paths(self._h, first, count,
                                       out.ctypes.data_as(C.POINTER(PathRecord))))
        return out

    def trace_launch(self, n: int) -> np.ndarray:
        """The production wave-pool launch of the current range (n path ids)
        with per-path final records (cvr_trace_launch)."""
        out = np.zeros(n, PATH_RECORD_DTYPE)
        self._c(load().cvr_trace_launch(self._h, out.ctypes.data_as(C.POINTER(PathRecord)), n))
        return out

    def device_info(self):
        cu, grid = C.c_int(), C.c_int()
        self._c(load().cvr_device_info(self._h, C.byref(cu), C.byref(grid)))
        return cu.value, grid.value

    def render_image(self, width, height, n_tiles=(1, 1), iterations=20, device_image: Optional[int] = None,
                     host: bool = True):
        return self.render_tiles(width, height, n_tiles, iterations, 0, 1, device_image, host)

    def render_frame(self, host_ptr=None, parts: int = 0, stats: bool = True,
                     host_floats: Optional[int] = None):
        """CudaVolPath::render for one tile (cvr_render_frame): clear, render
        the set resolution / iterations, and the normalised image in host
        memory when it returns, the launch split into `parts` bands whose
        copies overlap the later bands.  host_ptr: a PinnedImage, or the
        address of a float buffer (pinned for asynchronous copies) together
        with host_floats, the floats it holds (the library rejects a buffer
        shorter than the tile); None returns a new array.  stats=False skips
        the counters (one synchronous read per band)."""
        st = Stats() if stats else None
        img = None
        w, h = self.resolution  # the library's own tile size (what cvr_render_frame writes)
        if host_ptr is None:
            if w == 0 or h == 0:
                raise CvrError(-3, "render_frame: no resolution set")
            img = np.zeros((h, w, 4), np.float32)
            host_ptr = img.ctypes.data
            host_floats = img.size
        elif isinstance(host_ptr, PinnedImage):
            host_floats = host_ptr.floats if host_floats is None else host_floats
            host_ptr = host_ptr.ptr.value
        elif host_floats is None:
            # a bare address says nothing about its size: the caller states it, so the library's
            # size check (ABI 3) always runs
            raise CvrError(-1, "render_frame: host_floats is required with a raw host_ptr")
        self._c(load().cvr_render_frame(self._h, C.c_void_p(host_ptr), host_floats, parts,
                                        C.byref(st) if stats else None))
        return img, st

    def frame_flush_info(self):
        """(blocks the last render_frame's flusher waves stored in the launch, 0 if it
        copied after the launch; calls that fell back to the copy) (cvr_frame_flush_info)."""
        b, f = C.c_uint32(0), C.c_uint32(0)
        self._c(load().cvr_frame_flush_info(self._h, C.byref(b), C.byref(f)))
        return b.value, f.value

    def last_wpool(self):
        """((eps, waves, med, record, flush), grid in waves) of the context's last wave-pool launch
        (cvr_debug_last_wpool); CvrError -3 before any."""
        inst, grid = (C.c_int32 * 5)(), C.c_uint32(0)
        self._c(load().cvr_debug_last_wpool(self._h, inst, C.byref(grid)))
        return tuple(int(v) for v in inst), grid.value

    def render_share_to_host(self, host_ptr: int, host_floats: int, width, height, n_tiles=(1, 1), iterations=20,
                             first_tile: int = 0, tile_stride: int = 1):
        """One device's share of a multi-device render (cvr_render_share_to_host):
        tiles first_tile, first_tile + tile_stride, ... (more than one tile), else
        this context's block shard, stored normalised into the full pinned host
        image at host_ptr (width*height*4 floats, e.g. a PinnedImage)."""
        d = RenderDesc()
        d.resolution[:] = (width, height)
        d.n_tiles[:] = n_tiles
        d.iterations = iterations
        st = Stats()
        self._c(load().cvr_render_share_to_host(self._h, C.byref(d), first_tile, tile_stride, C.c_void_p(host_ptr),
                                                host_floats, C.byref(st)))
        return st

    def render_tiles(self, width, height, n_tiles=(1, 1), iterations=20, first_tile: int = 0,
                     tile_stride: int = 1, device_image: Optional[int] = None, host: bool = True):
        """Tiles first_tile, first_tile + tile_stride, ... of render_image's
        tile loop, each with its sequential-loop seed (cvr_render_tiles)."""
        d = RenderDesc()
        d.resolution[:] = (width, height)
        d.n_tiles[:] = n_tiles
        d.iterations = iterations
        st = Stats()
        img = np.zeros((height, width, 4), np.float32) if host else None
        self._c(load().cvr_render_tiles(self._h, C.byref(d), first_tile, tile_stride,
                                        C.c_void_p(device_image) if device_image else None,
                                        _fp(img) if host else None, C.byref(st)))
        return img, st

    def close(self):
        if getattr(self, "_h", None):
            load().cvr_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()


def _adaptive_maps(ctx: Context):
    """(block error map f64, block samples map u32), (tile_h / 8, tile_w / 8) (cvr_adaptive_maps)."""
    w, h = ctx.resolution
    err = np.zeros((h // 8, w // 8), np.float64)
    smp = np.zeros((h // 8, w // 8), np.uint32)
    ctx._c(load().cvr_adaptive_maps(ctx._h, err.ctypes.data_as(C.POINTER(C.c_double)),
                                    smp.ctypes.data_as(C.POINTER(C.c_uint32))))
    return err, smp


class AdaptiveSession:
    """An open adaptive render of a Context (Context.adaptive): step() runs one pass, maps() gives
    every block's last error and sample count, image() the image normalised per block."""

    def __init__(self, ctx: Context, desc: AdaptiveDesc):
        self.ctx = ctx
        self.desc = desc
        self.open = False
        self.result = None
        self.stats = Stats()  # summed counters of the passes so far

    def __enter__(self):
        self.ctx._c(load().cvr_adaptive_begin(self.ctx._h, C.byref(self.desc)))
        self.open = True
        return self

    def __exit__(self, *exc):
        if self.open:
            self.open = False
            self.ctx._c(load().cvr_adaptive_end(self.ctx._h))
        return False

    def step(self) -> AdaptiveResult:
        res = AdaptiveResult()
        self.ctx._c(load().cvr_adaptive_pass(self.ctx._h, C.byref(res)))
        s = self.ctx.stats()  # the pass's launch
        for k in ("paths", "segments", "steps", "density", "albedo", "escaped", "truncated", "fetches"):
            setattr(self.stats, k, getattr(self.stats, k) + getattr(s, k))
        self.stats.kernel_ms += s.kernel_ms
        self.result = res
        return res

    def maps(self):
        return _adaptive_maps(self.ctx)

    def image(self, host_ptr=None) -> np.ndarray:
        w, h = self.ctx.resolution
        if isinstance(host_ptr, PinnedImage):
            self.ctx._c(load().cvr_adaptive_image(self.ctx._h, host_ptr.ptr, host_ptr.floats))
            return host_ptr.array
        img = np.zeros((h, w, 4), np.float32)
        self.ctx._c(load().cvr_adaptive_image(self.ctx._h, C.c_void_p(img.ctypes.data), img.size))
        return img

    def denoised(self, desc: Optional[DenoiseDesc] = None, host_ptr=None) -> np.ndarray:
        """The session's image filtered with its moments, every block at its own sample count
        (Context.denoise inside the session)."""
        return self.ctx.denoise(desc, None, host_ptr)

    def denoised_guided(self, desc: Optional[DenoiseGuidedDesc] = None, features: Optional[FeaturesDesc] = None,
                        host_ptr=None) -> np.ndarray:
        """The session's image so far through the feature-guided filter (Context.denoise_guided
        inside the session)."""
        return self.ctx.denoise_guided(desc, None, features, host_ptr)


class PinnedImage:
    """A width x height float4 image in pinned, device-mapped host memory
    (cvr_host_alloc), viewed as a numpy array; every device can store into it."""

    def __init__(self, width: int, height: int):
        self.ptr = C.c_void_p()
        rc = load().cvr_host_alloc(width * height * 16, C.byref(self.ptr))
        if rc != 0:
            raise CvrError(rc, load().cvr_last_error(None).decode())
        self.floats = width * height * 4
        self.array = np.ctypeslib.as_array(C.cast(self.ptr, C.POINTER(C.c_float)), shape=(height, width, 4))

    def close(self):
        if self.ptr:
            load().cvr_host_free(self.ptr)
            self.ptr = C.c_void_p()
            self.array = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False

    def __del__(self):
        try:
            self.close()
        except Exception:  # noqa: BLE001 (interpreter shutdown: the library may be gone)
            pass
