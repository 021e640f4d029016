"""The clip region's host statement (cvr_clip_host) against its numpy restatement, the descriptor's
refusals and its size; no GPU.

tests/clip_ref.py evaluates cvr.h's statement with float32 operations in the stated order, on its
own; every case compares the kept mask, the density and the albedo bit for bit.  A context needs a
device, so the refusals are driven through cvr_clip_host, which checks the descriptor as
cvr_set_clip does (one function behind both); cvr_set_clip itself, cvr_get_clip's round trip and
the adaptive-session guard run in tests/test_gpu_clip.py.  `make clip-host-asan` runs the statement
over the same ragged cases under AddressSanitizer and UBSan (tests/cpp/clip_host_check.cpp)."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import clip_ref as cr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID = -1


def host(cvr, region, res=cr.RES, density=None, albedo=None):
    return cvr.clip_host(res, region.lo, region.hi, region.planes, density, albedo)


@pytest.mark.parametrize("name", sorted(cr.CPU_REGIONS))
def test_clip_host_equals_the_numpy_statement(cvr, name):
    region = cr.CPU_REGIONS[name]
    d, a = cr.arrays()
    keep, dn, al = host(cvr, region, density=d, albedo=a)
    rk, rd, ra = cr.clip(d, a, region)
    assert keep.dtype == np.uint8 and set(np.unique(keep)) <= {0, 1}
    mism = np.argwhere(keep.astype(bool) != rk)
    assert mism.size == 0, f"{name}: {len(mism)} voxels decided otherwise, first (z, y, x) {mism[:3].tolist()}"
    assert dn.tobytes() == rd.tobytes() and al.tobytes() == ra.tobytes(), name
    # a kept voxel is untouched, a clipped one is (+0, voxel 0's albedo)
    assert dn[rk].tobytes() == d[rk].tobytes() and al[rk].tobytes() == a[rk].tobytes()
    assert not dn[~rk].view(np.uint32).any() and (al[~rk] == a[0, 0, 0]).all()


def test_the_regions_cut_what_their_names_say(cvr):
    """The cases are not vacuous: counts by reasoning, not from the code under test."""
    nx, ny, nz = cr.RES
    n = nx * ny * nz
    count = {k: int(host(cvr, r)[0].sum()) for k, r in cr.CPU_REGIONS.items()}
    assert count["crop"] == (30 - 3) * (17 - 9) * (nz - 2)          # hi[2] = 40 means "to the end"
    assert count["empty_crop"] == 0 and count["keep_none"] == 0 and count["keep_all"] == n
    assert count["lattice_tie"] == sum(min(x + 1, ny) for x in range(nx)) * nz   # y <= x, the tie x == y kept
    assert count["neg_zero_d"] == nx * nz                             # the plane y == 0 alone: t = +-0 is kept
    assert 0 < count["oblique"] < n and 0 < count["slab"] < n and 0 < count["eight"] < count["slab"]
    keep = host(cvr, cr.LATTICE_TIE)[0]
    assert keep[3, 5, 5] == 1 and keep[3, 6, 5] == 0 and keep[3, 4, 5] == 1


def test_each_array_may_be_absent_and_voxel_zero_follows_the_rule(cvr):
    d, a = cr.arrays()
    region = cr.Region((1, 0, 0), None)                               # voxel 0 itself is clipped
    keep, dn, al = host(cvr, region, density=d, albedo=a)
    assert keep[0, 0, 0] == 0 and dn[0, 0, 0] == 0 and al[0, 0, 0].tobytes() == a[0, 0, 0].tobytes()
    assert al[5, 5, 0].tobytes() == a[0, 0, 0].tobytes() and al[5, 5, 1].tobytes() == a[5, 5, 1].tobytes()
    k2, d2, a2 = host(cvr, region, density=d)
    assert a2 is None and d2.tobytes() == dn.tobytes() and k2.tobytes() == keep.tobytes()
    k3, d3, a3 = host(cvr, region, albedo=a)
    assert d3 is None and a3.tobytes() == al.tobytes()
    lib = cvr.load()
    desc = cvr.ClipDesc()
    desc.hi[:] = (4, 4, 4)
    res = (C.c_uint32 * 3)(5, 4, 3)
    assert lib.cvr_clip_host(res, C.byref(desc), None, None, None) == 0   # nothing to write: still checked
    assert lib.cvr_clip_host(None, C.byref(desc), None, None, None) == INVALID
    assert lib.cvr_clip_host((C.c_uint32 * 3)(5, 0, 3), C.byref(desc), None, None, None) == INVALID


def refusal(cvr, desc):
    lib = cvr.load()
    keep = np.zeros(60, np.uint8)
    code = lib.cvr_clip_host((C.c_uint32 * 3)(5, 4, 3), None if desc is None else C.byref(desc), None, None,
                             keep.ctypes.data)
    return code, (lib.cvr_last_error(None) or b"").decode()


def bad_desc(*faults):
    """A descriptor with the given faults, each later in the header's order than the one before."""
    d = cvr_desc()
    for f in faults:
        if f == "flags":
            d.flags = 4
        elif f == "n_planes":
            d.n_planes = 9
        elif f == "lo_hi":
            d.lo[1], d.hi[1] = 7, 6
        elif f == "non_finite":
            d.n_planes = max(d.n_planes, 2)
            d.planes[1][3] = float("inf")
        elif f == "zero_normal":
            d.n_planes = max(d.n_planes, 1)
            d.planes[0][:] = (0.0, 0.0, 0.0, 1.0)
    return d


def cvr_desc():
    import cudavolumerenderer_amd as cvr
    d = cvr.ClipDesc()
    d.hi[:] = (0xFFFFFFFF,) * 3
    d.n_planes = 2
    d.planes[0][:] = (1.0, 0.0, 0.0, 0.0)
    d.planes[1][:] = (0.0, 1.0, 0.0, 0.0)
    return d


ORDER = [("flags", "flags"), ("n_planes", "clip planes"), ("lo_hi", "crop lo"), ("non_finite", "not finite"),
         ("zero_normal", "zero normal")]


def test_the_six_refusals_in_the_headers_order(cvr):
    assert refusal(cvr, cvr_desc())[0] == 0
    code, msg = refusal(cvr, None)
    assert code == INVALID and "NULL" in msg
    # each fault alone, and each fault with every later one present: the earlier one is named
    for i, (fault, words) in enumerate(ORDER):
        later = [f for f, _ in ORDER[i + 1:]]
        if fault == "n_planes":
            later = [f for f in later if f not in ("non_finite", "zero_normal")]  # (they would lower n_planes' claim)
        for faults in ([fault], [fault] + later):
            code, msg = refusal(cvr, bad_desc(*faults))
            assert code == INVALID and words in msg, (faults, msg)
    # n_planes = 9 beside a bad plane entry
    d = bad_desc("zero_normal", "non_finite")
    d.n_planes = 9
    assert "clip planes" in refusal(cvr, d)[1]
    # entries from n_planes on are ignored; -inf and NaN are refused like +inf; an empty crop is allowed
    d = cvr_desc()
    d.planes[5][:] = (0.0, 0.0, 0.0, float("nan"))
    assert refusal(cvr, d)[0] == 0
    for v in (float("-inf"), float("nan")):
        d = cvr_desc()
        d.planes[0][1] = v
        assert "not finite" in refusal(cvr, d)[1]
    d = cvr_desc()
    d.lo[:], d.hi[:] = (2, 2, 2), (2, 2, 2)
    assert refusal(cvr, d)[0] == 0
    lib = cvr.load()
    assert lib.cvr_set_clip(None, C.byref(cvr_desc())) == INVALID and lib.cvr_clear_clip(None) == INVALID
    assert lib.cvr_get_clip(None, None, None) == INVALID and lib.cvr_medium_clip_info(None, None, None) == INVALID


def test_descriptor_size_matches_the_headers_comment(cvr):
    text = open(os.path.join(ROOT, "include", "cvr.h")).read()
    m = re.search(r"\}\s*cvr_clip_desc;\s*/\*\s*(\d+) bytes\s*\*/", text)
    assert m and int(m.group(1)) == C.sizeof(cvr.ClipDesc) == 160
    assert "#define CVR_HAS_CLIP 1" in text and "#define CVR_CLIP_MAX_PLANES 8" in text
    assert cvr.CLIP_MAX_PLANES == 8
    # the C compiler agrees
    cc = shutil.which("cc") or shutil.which("gcc")
    if cc:
        src = '#include "cvr.h"\n_Static_assert(sizeof(cvr_clip_desc) == 160, "size");\nint main(void){return 0;}\n'
        subprocess.run([cc, "-fsyntax-only", "-I", os.path.join(ROOT, "include"), "-x", "c", "-"], input=src.encode(),
                       check=True)


def test_plane_from_box_maps_box_coordinates_to_indices(cvr):
    """(p - min) / extent * (res - 1): the plane through the box's centre keeps the upper half."""
    res = (65, 33, 17)
    lo, hi = (-1.0, 0.0, 2.0), (1.0, 4.0, 3.0)
    A, B, Cc, D = cvr.plane_from_box((0.0, 2.0, 2.5), (1.0, 0.0, 0.0), lo, hi, res)
    assert (A, B, Cc, D) == (np.float32(2.0 / 64), 0.0, 0.0, np.float32(-1.0)) and A * np.float32(32) + D == 0
    keep = cvr.clip_host(res, planes=[(A, B, Cc, D)])[0]
    assert keep[:, :, 32:].all() and not keep[:, :, :32].any()
    # an oblique one: voxel centres on the positive side of the plane in box space are kept
    p, n = np.array([0.1, 1.7, 2.4]), np.array([0.3, -0.8, 0.52])
    keep = cvr.clip_host(res, planes=[cvr.plane_from_box(p, n, lo, hi, res)])[0].astype(bool)
    z, y, x = np.meshgrid(*(np.arange(v) for v in res[::-1]), indexing="ij")
    pos = np.stack([lo[k] + c / (res[k] - 1.0) * (hi[k] - lo[k]) for k, c in enumerate((x, y, z))], -1)
    s = (pos - p) @ n
    sure = np.abs(s) > 1e-4                                   # (float32 coefficients: leave the plane itself out)
    assert (keep[sure] == (s[sure] > 0)).all() and 0.2 < keep.mean() < 0.8



# --------------------------------------------------------------------- CLI --
CLI = os.path.join(ROOT, "cudavolumerenderer_amd", "cvr")


def test_cli_crop_and_clip_plane_argument_errors(tmp_path):
    """Every one is found before a device is touched; VDB, MHD and XML scenes have no bytes to clip."""
    good = tmp_path / "good.txt"
    good.write_text("# n m\n2 2\n\n0 0 0 0\n1 0.5 0.25 1\n# row 1\n0 0 0 0.5\n1 1 1 1\n")
    tf2d = ("--transfer2d", str(good), "--gradient-range", "0", "100")

    def err_of(*args):
        r = subprocess.run([CLI, "--interactive", "0", *args], capture_output=True, text=True, timeout=120)
        assert r.returncode == 2 and "[ConfigParser] Error:" in r.stderr, (args, r.returncode, r.stderr)
        return r.stderr

    crop = ("--crop", "1", "2", "3", "20", "21", "22")
    assert "--crop needs 6 values" in err_of("--synthetic", "bucky", *tf2d, "--crop", "1", "2", "3")
    assert "--clip-plane needs 4 values" in err_of("--synthetic", "bucky", *tf2d, "--clip-plane", "1", "0", "--pfm")
    assert "apply to Raw scenes only" in err_of("--synthetic", "hetvol", *crop)   # (no scalar bytes: as VDB, MHD, XML)
    assert "need --transfer or --transfer2d" in err_of("--synthetic", "bucky", *crop)
    assert "need --transfer or --transfer2d" in err_of("--synthetic", "bucky", "--clip-plane", "1", "0", "0", "-3.5")
    nine = [v for _ in range(9) for v in ("--clip-plane", "1", "0", "0", "-3.5")]
    assert "at most 8 --clip-plane" in err_of("--synthetic", "bucky", *tf2d, *nine)
    assert "zero normal" in err_of("--synthetic", "bucky", *tf2d, "--clip-plane", "0", "0", "0", "1")
    assert "crop lo" in err_of("--synthetic", "bucky", *tf2d, "--crop", "9", "0", "0", "8", "32", "32")
    assert "not finite" in err_of("--synthetic", "bucky", *tf2d, "--clip-plane", "1", "nan", "0", "1")
    # a crop takes voxel indices: a negative number, a word or more than 2^32 - 1 is refused, not wrapped
    for bad in ("-1", "abc", "7x", "4294967296", "1.5"):
        assert "is not a voxel index" in err_of("--synthetic", "bucky", *tf2d, "--crop", "0", "0", "0", "9", bad, "9"), bad
    assert "is not a number" in err_of("--synthetic", "bucky", *tf2d, "--clip-plane", "1", "0", "zero", "1")
