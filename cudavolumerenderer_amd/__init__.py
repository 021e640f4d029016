"""MI355X-native volumetric path tracer (the hot path of Fe0437/CudaVolumeRenderer).

The renderer is libcvr.so (HIP for gfx950 behind the C ABI in include/cvr.h);
this package is its ctypes binding plus the multi-GPU driver.  There is no
CPU fallback: on a machine without a GPU, Context() raises.
"""
from ._lib import (  # noqa: F401
    KERNELS, NAIVE_SK, NAIVE_MK, REGENERATION_SK, STREAMING_MK, STREAMING_SK, SORTING_SK,
    OPT_MAX_SEGMENTS, OPT_CHUNK, OPT_EVENT_THRESHOLD, OPT_GRID, OPT_SCATTER_EPS,
    OPT_SCHEDULER, OPT_POOL, OPT_TIMING, OPT_CELLS, OPT_WAVES, OPT_ORDER, OPT_QUEUES, OPT_BOUNDS, OPT_TAIL, OPT_BATCH, OPT_RNG_BINDING, OPT_MORTON, OPT_WORLD_TO_AABB, OPT_MK_COMPACTION, OPT_SUBQUEUES, OPT_DRAIN, OPT_INFLIGHT, OPT_FRAME_FLUSH, OPT_UNIFORM_ALBEDO, OPT_WAVE_PAIR, OPT_SAMPLE_ORDER, OPT_EMPTY_MASK, OPT_COUNT_WORDS,
    OPT_MEDIUM_FORMAT, FORMAT_F32, FORMAT_F16, MediumInfo, half_round,
    OPT_MOMENTS, AdaptiveDesc, AdaptiveResult, AdaptiveSession, block_error,
    DenoiseDesc, denoise_host,
    FeaturesDesc, DenoiseGuidedDesc, features_host, denoise_guided_host,
    PreviewDesc, PREVIEW_UNSHADED, PREVIEW_HEADLIGHT, preview_host,
    LightVolumeDesc, LightVolumeInfo, light_volume_host, preview_shadowed_host,
    DeviceMediumDesc, MediumLayout, DEVMED_SPARSE, DEVMED_CONST_ALBEDO, DEVMED_MAX_DENSITY,
    MEDIUM_ARRAYS, build_geometry, wpool_rows,
    TransferDesc, ScalarMediumDesc, classify_host, raw_transfer_table,
    GradientTransferDesc, GradientMediumDesc, classify_gradient_host,
    LabelTransferDesc, LabeledMediumDesc, classify_labels_host,
    ClipDesc, CLIP_MAX_PLANES, clip_host, plane_from_box,
    FieldDesc, HistogramDesc, FieldStats, field_stats_host, field_histogram_host, field_geometry,
    ProjectDesc, PROJECT_MAX, PROJECT_MIN, PROJECT_MEAN, PROJECT_ISO, PROJECT_HEADLIGHT, field_project_host,
    SCALAR_F32, SCALAR_U8, SCALAR_U16, SCALAR_I16, TF_CEIL, TF_DENSITY_U,
    EnvironmentDesc, EnvironmentInfo, ENV_HOST, ENV_DEVICE, ENV_RECORD_DTYPE, environment_eval_host,
    environment_eval_host_fn, read_image, rotation_y,
    PATH_RECORD_DTYPE, CvrError, Context, MediumDesc, PinnedImage, Scene, Stats, default_camera, load,
    medium_from_arrays, tile_origin, tiling, write_hdr, LIB_PATH,
)

__all__ = [
    "KERNELS", "Context", "Scene", "MediumDesc", "Stats", "CvrError", "PinnedImage", "default_camera", "tiling",
    "tile_origin", "write_hdr", "medium_from_arrays", "load", "LIB_PATH", "PATH_RECORD_DTYPE",
    "OPT_MEDIUM_FORMAT", "FORMAT_F32", "FORMAT_F16", "MediumInfo", "half_round",
    "OPT_MOMENTS", "AdaptiveDesc", "AdaptiveResult", "AdaptiveSession", "block_error",
    "DenoiseDesc", "denoise_host",
    "FeaturesDesc", "DenoiseGuidedDesc", "features_host", "denoise_guided_host",
    "PreviewDesc", "PREVIEW_UNSHADED", "PREVIEW_HEADLIGHT", "preview_host",
    "LightVolumeDesc", "LightVolumeInfo", "light_volume_host", "preview_shadowed_host",
    "DeviceMediumDesc", "MediumLayout", "DEVMED_SPARSE", "DEVMED_CONST_ALBEDO", "DEVMED_MAX_DENSITY",
    "MEDIUM_ARRAYS", "build_geometry", "wpool_rows",
    "TransferDesc", "ScalarMediumDesc", "classify_host", "raw_transfer_table",
    "GradientTransferDesc", "GradientMediumDesc", "classify_gradient_host",
    "LabelTransferDesc", "LabeledMediumDesc", "classify_labels_host",
    "ClipDesc", "CLIP_MAX_PLANES", "clip_host", "plane_from_box",
    "FieldDesc", "HistogramDesc", "FieldStats", "field_stats_host", "field_histogram_host", "field_geometry",
    "ProjectDesc", "PROJECT_MAX", "PROJECT_MIN", "PROJECT_MEAN", "PROJECT_ISO", "PROJECT_HEADLIGHT", "field_project_host",
    "SCALAR_F32", "SCALAR_U8", "SCALAR_U16", "SCALAR_I16", "TF_CEIL", "TF_DENSITY_U",
    "EnvironmentDesc", "EnvironmentInfo", "ENV_HOST", "ENV_DEVICE", "ENV_RECORD_DTYPE", "environment_eval_host",
    "environment_eval_host_fn", "read_image", "rotation_y",
]
