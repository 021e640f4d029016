"""Media from device memory (cvr_set_medium_device), the parts that need no GPU: the ABI surface,
the header's ABI 5 view, the Python wrapper's argument checks, and the numpy statement of the leaf
rule (tests/devmed.py) that tests/test_gpu_device_medium.py builds its host-side references with."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import devmed
import media

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ----------------------------------------------------------------- surface --
def test_surface(cvr):
    lib = cvr.load()
    for name in ("cvr_set_medium_device", "cvr_medium_layout"):
        assert hasattr(lib, name), name
    assert C.sizeof(cvr.DeviceMediumDesc) == 96
    assert [f for f, _ in cvr.DeviceMediumDesc._fields_] == [
        "res", "flags", "d_density", "d_albedo", "const_albedo", "box_min", "box_max", "scale", "max_density", "g",
        "roughness", "eta"]
    assert [getattr(cvr.DeviceMediumDesc, f).offset for f in ("res", "flags", "d_density", "d_albedo", "const_albedo",
                                                               "box_min", "box_max", "scale", "eta")] == \
        [0, 12, 16, 24, 32, 48, 60, 72, 92]
    assert C.sizeof(cvr.MediumLayout) == 6 * 4 + 3 * 4 + 64 * 4
    assert (cvr.DEVMED_SPARSE, cvr.DEVMED_CONST_ALBEDO, cvr.DEVMED_MAX_DENSITY) == (1, 2, 4)
    hdr = open(os.path.join(ROOT, "include", "cvr.h")).read()
    assert "#define CVR_HAS_DEVICE_MEDIUM 1" in hdr
    assert lib.cvr_abi_version() == 6  # an addition within ABI 6


def test_header_hides_device_medium_from_abi5(tmp_path):
    def compiles(src, *flags):
        f = tmp_path / "t.c"
        f.write_text('#include "cvr.h"\n' + src)
        r = subprocess.run(["cc", "-std=c11", "-Werror", "-Wall", "-fsyntax-only", "-I", os.path.join(ROOT, "include"),
                            *flags, str(f)], capture_output=True, text=True, timeout=60)
        return r.returncode == 0, r.stderr

    use = ("#ifndef CVR_HAS_DEVICE_MEDIUM\n#error \"no device medium\"\n#endif\n"
           "_Static_assert(sizeof(cvr_device_medium_desc) == 96, \"96 bytes\");\n"
           "int f(cvr_ctx* c, const float* p) { cvr_device_medium_desc d = {{8, 8, 8}, CVR_DEVMED_SPARSE |\n"
           "  CVR_DEVMED_CONST_ALBEDO | CVR_DEVMED_MAX_DENSITY, p, 0, {1, 1, 1, 1}, {0, 0, 0}, {1, 1, 1}, 100.0f, 0.0f,\n"
           "  0.0f, {0.1f, 0.1f}, 1.04f}; struct cvr_medium_layout l;\n"
           "  return cvr_set_medium_device(c, &d) + cvr_medium_layout(c, &l) + (int)l.mask[63]; }\n")
    ok, err = compiles(use)
    assert ok, err
    assert compiles(use, "-DCVR_ABI_TARGET=6")[0]
    ok, err = compiles("cvr_device_medium_desc d;\n", "-DCVR_ABI_TARGET=5")
    assert not ok and "cvr_device_medium_desc" in err
    ok, err = compiles("struct cvr_medium_layout l;\n", "-DCVR_ABI_TARGET=5")
    assert not ok and "cvr_medium_layout" in err
    ok, _ = compiles("#ifdef CVR_HAS_DEVICE_MEDIUM\n#error \"declared\"\n#endif\n", "-DCVR_ABI_TARGET=5")
    assert ok


# ------------------------------------------------- the wrapper's own checks --
class FakeDevice:
    def __init__(self, kind="cuda", index=0):
        self.type, self.index = kind, index

    def __str__(self):
        return f"{self.type}:{self.index}"


class FakeTensor:
    """What the wrapper looks at of a tensor; data_ptr() fails the test if the library is reached."""

    def __init__(self, shape, dtype="torch.float32", contiguous=True, device=None):
        self.shape, self.dtype, self._contiguous = shape, dtype, contiguous
        self.device = FakeDevice() if device is None else device

    def is_contiguous(self):
        return self._contiguous

    def data_ptr(self):
        raise AssertionError("the library call was prepared before the arguments were checked")


def test_wrapper_checks_arguments_first(cvr):
    ctx = cvr.Context.__new__(cvr.Context)  # no GPU: no library context behind it
    ctx._h, ctx.device = None, 0
    good_d, good_a = FakeTensor((4, 5, 6)), FakeTensor((4, 5, 6, 4))
    bad = [
        ("dtype", dict(density=FakeTensor((4, 5, 6), dtype="torch.float16"), albedo=good_a)),
        ("dtype", dict(density=good_d, albedo=FakeTensor((4, 5, 6, 4), dtype="torch.float64"))),
        ("contiguous", dict(density=FakeTensor((4, 5, 6), contiguous=False), albedo=good_a)),
        ("contiguous", dict(density=good_d, albedo=FakeTensor((4, 5, 6, 4), contiguous=False))),
        ("shape", dict(density=FakeTensor((4, 5)), albedo=good_a)),
        ("shape", dict(density=good_d, albedo=FakeTensor((4, 5, 6, 3)))),
        ("shape", dict(density=good_d, albedo=FakeTensor((6, 5, 4, 4)))),
        ("cuda:0", dict(density=FakeTensor((4, 5, 6), device=FakeDevice("cuda", 1)), albedo=good_a)),
        ("cuda:0", dict(density=good_d, albedo=FakeTensor((4, 5, 6, 4), device=FakeDevice("cpu", None)))),
        ("exactly one", dict(density=good_d, albedo=good_a, const_albedo=(1, 1, 1, 1))),
        ("exactly one", dict(density=good_d)),
        ("4 floats", dict(density=good_d, const_albedo=(1, 1, 1))),
        ("res", dict(density=1 << 20, const_albedo=(1, 1, 1, 1))),
    ]
    for word, kw in bad:
        with pytest.raises(ValueError) as e:
            ctx.set_medium_device(**kw)
        assert word in str(e.value), (word, str(e.value))
    ctx._h = None


# ------------------------------------------------------------ the leaf rule --
def assert_same_leaves(sp, table, dens, alb, bg, what):
    assert np.array_equal(sp.table, table), what
    assert np.array_equal(sp.leaf_density.view(np.uint32), dens.reshape(-1, 512).view(np.uint32)), what
    assert (sp.leaf_albedo is None) == (alb is None), what
    if alb is not None:
        assert np.array_equal(sp.leaf_albedo.view(np.uint32), alb.reshape(-1, 512, 4).view(np.uint32)), what
    assert np.array_equal(np.array(sp.albedo_bg, np.float32).view(np.uint32), np.asarray(bg, np.float32).view(np.uint32))


@pytest.mark.parametrize("name,dims", [("bucky", None), ("manix", (64, 58, 64)), ("manix", (20, 12, 28)),
                                       ("hetvol", (40, 33, 17))])
def test_leaf_rule_equals_the_scene_builder(cvr, name, dims):
    """cvr_scene_sparse_medium on a dense synthetic scene and the numpy rule on its grids."""
    s = cvr.Scene.synthetic(name, 0, dims)
    assert not s.is_sparse
    table, dens, alb, bg = s.leaves()
    assert_same_leaves(devmed.leaf_rule(s.density, s.albedo), table, dens, alb, bg, name)


def test_leaf_rule_on_a_scene_with_the_planted_voxels(cvr):
    """The scene builder never sees -0, NaN or an albedo-only leaf in its synthetic scenes: the
    rule's words for them are checked on the planted grids themselves."""
    for name, with_albedo in (("sparse_small", True), ("sparse_small", False), ("sparse_es4", True)):
        D, A, md = devmed.sparse_grid(name, with_albedo)
        src = media.sparse_small(with_albedo) if name == "sparse_small" else media.sparse_es4()
        sp = devmed.leaf_rule(D, A)
        present = sp.table != devmed.NO_LEAF
        want = src.table != devmed.NO_LEAF
        plants = devmed.PLANTS[name]
        for kind, (x, y, z) in plants.items():
            want[z, y, x] = kind in ("nan", "corner") or (kind == "albedo" and with_albedo)
        assert np.array_equal(present, want), name
        assert (sp.leaf_albedo is not None) == with_albedo
        assert np.array_equal(sp.table[present], np.arange(present.sum()))  # z, y, x order, x fastest
        # the leaves hold the grid: densifying them gives it back, bit for bit (NaN and all but the
        # -0, whose leaf is not stored)
        D2, A2 = devmed.densify(sp)
        x, y, z = plants["negzero"]
        D0 = D.copy()
        D0[8 * z + 1, 8 * y + 2, 8 * x + 1] = 0.0
        assert np.array_equal(D2.view(np.uint32), D0.view(np.uint32)), name
        assert np.array_equal(A2.view(np.uint32), A.view(np.uint32)), name
        # padding voxels of stored leaves: density 0, the background's albedo
        if name == "sparse_small":
            nx, ny, nz = sp.res
            pool = sp.leaf_density.reshape(-1, 8, 8, 8)
            slot = sp.table[0, 1, 0]           # leaf (0, 1, 0): y = 8..15 of ny = 12
            assert slot != devmed.NO_LEAF and (pool[slot][:, 4:, :] == 0).all() and (pool[slot][:, :4, :] != 0).any()
            if with_albedo:
                pa = sp.leaf_albedo.reshape(-1, 8, 8, 8, 4)
                assert (pa[slot][:, 4:, :] == np.array(sp.albedo_bg, np.float32)).all()


def test_centre_voxel_medium_is_sharp(cvr, oracle_mod):
    """The oracle's records over the centre-voxel medium differ from those over its uniform
    version, so a device scan that called this albedo uniform could not pass the GPU test."""
    m = devmed.centre_voxel()
    ref = devmed.dense_reference("centre_voxel", 0)
    flat = m.albedo.copy()
    flat[..., :3] = np.float32(0.9)
    uni = devmed.oracle_records(m.density, flat, m.max_density, 0, m.box_min, m.box_max, m.scale)
    differ = (ref["T"].view(np.uint32) != uni["T"].view(np.uint32)).any(axis=1)
    assert differ.sum() >= 16, differ.sum()
    assert (ref["flags"] & 1).any() and (ref["n_albedo"] > 0).any()
