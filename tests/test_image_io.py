"""cvr_read_image (csrc/cvr_image_io.cpp): Radiance .hdr (flat and new-style run-length encoded
scanlines) and colour .pfm (both byte orders) into RGB floats, row 0 the top; malformed files are
CVR_ERR_IO.  No GPU.

The same files also go through tests/cpp/image_io_san.cpp, a stand-alone program built here from
the reader's source alone with g++ -fsanitize=address,undefined: a read or write outside a
buffer, or undefined arithmetic on a header's numbers, ends that program with a report."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CVR_ERR_IO = -4
HDR_HEAD = b"#?RADIANCE\nFORMAT=32-bit_rle_rgbe\n\n"


def rgbe_encode(rgb):
    """cvr_write_hdr's encoding (stb's), restated: (h, w, 3) float32 -> (h, w, 4) uint8."""
    f = np.float32
    mx = rgb.max(axis=-1)
    m, ex = np.frexp(mx)
    out = np.zeros(rgb.shape[:2] + (4,), np.uint8)
    ok = mx >= f(1e-32)
    nrm = np.where(ok, m.astype(f) * f(256) / np.where(ok, mx, f(1)), f(0)).astype(f)
    out[..., :3] = np.where(ok[..., None], (rgb * nrm[..., None]).astype(f), f(0)).astype(np.uint8)
    out[..., 3] = np.where(ok, ex + 128, 0).astype(np.uint8)
    return out


def rgbe_decode(e):
    """(h, w, 4) uint8 -> float32: byte * 2^(e - 136), e = 0 black (the reader's stated convention)."""
    scale = np.ldexp(np.float32(1), e[..., 3].astype(np.int32) - 136).astype(np.float32)
    return np.where(e[..., 3:4] > 0, e[..., :3].astype(np.float32) * scale[..., None], np.float32(0)).astype(np.float32)


def rle_scanline(texels):
    """One new-style run-length encoded scanline of (w, 4) uint8 texels: runs of 3..127 equal bytes
    as (128 + n, value), everything else as literals of up to 128 bytes."""
    w = len(texels)
    out = bytearray([2, 2, w >> 8, w & 255])
    for ch in range(4):
        v = texels[:, ch].tolist()
        x = 0
        while x < w:
            run = 1
            while x + run < w and run < 127 and v[x + run] == v[x]:
                run += 1
            if run >= 3:
                out += bytes([128 + run, v[x]])
                x += run
                continue
            lit = []
            while x < w and len(lit) < 128:
                if x + 2 < w and v[x] == v[x + 1] == v[x + 2]:
                    break
                lit.append(v[x])
                x += 1
            out += bytes([len(lit)]) + bytes(lit)
    return bytes(out)


def picture(w=40, h=6, seed=9):
    rng = np.random.default_rng(seed)
    img = (rng.random((h, w, 3), dtype=np.float32) * np.float32(4.0)).astype(np.float32)
    img[1, 5:30] = img[1, 5]      # long runs in every channel
    img[2, :] = np.float32(0.0)   # a black scanline (e = 0)
    img[3, 10:13] = np.float32(1e-3)
    img[4, 0] = (1000.0, 0.5, 0.25)
    return img


def hdr_bytes(e, rle):
    h, w = e.shape[:2]
    body = b"".join(rle_scanline(e[y]) for y in range(h)) if rle else e.tobytes()
    return HDR_HEAD + b"-Y %d +X %d\n" % (h, w) + body


def pfm_bytes(img, little, scale=1.0):
    h, w = img.shape[:2]
    head = b"PF\n%d %d\n%s\n" % (w, h, repr(-scale if little else scale).encode())
    return head + img[::-1].astype("<f4" if little else ">f4").tobytes()


def test_written_hdr_reads_back_as_its_quantisation(cvr, tmp_path):
    img = picture()
    rgba = np.concatenate([img, np.ones(img.shape[:2] + (1,), np.float32)], axis=-1)
    p = tmp_path / "w.hdr"
    cvr.write_hdr(str(p), rgba)
    got = cvr.read_image(str(p))
    want = rgbe_decode(rgbe_encode(img))
    assert got.shape == img.shape and got.dtype == np.float32
    assert (got.view(np.uint32) == want.view(np.uint32)).all()
    # and the quantisation is RGBE's: within 2^-7 of the texel's largest component, from below
    assert (np.abs(got - img).max(axis=-1) <= img.max(axis=-1) * 2.0 ** -7 + 1e-30).all()


def test_rle_file_decodes_as_the_flat_file(cvr, tmp_path):
    e = rgbe_encode(picture())
    flat, rle = tmp_path / "flat.hdr", tmp_path / "rle.hdr"
    flat.write_bytes(hdr_bytes(e, False))
    rle.write_bytes(hdr_bytes(e, True))
    assert len(rle.read_bytes()) != len(flat.read_bytes())
    assert len(rle_scanline(e[1])) < 4 * e.shape[1]  # the encoder does emit runs
    a, b = cvr.read_image(str(flat)), cvr.read_image(str(rle))
    assert (a.view(np.uint32) == b.view(np.uint32)).all()
    assert (a.view(np.uint32) == rgbe_decode(e).view(np.uint32)).all()
    # a file may mix the two kinds of scanline
    mixed = tmp_path / "mixed.hdr"
    h, w = e.shape[:2]
    mixed.write_bytes(HDR_HEAD + b"-Y %d +X %d\n" % (h, w)
                      + b"".join(rle_scanline(e[y]) if y % 2 else e[y].tobytes() for y in range(h)))
    assert (cvr.read_image(str(mixed)).view(np.uint32) == a.view(np.uint32)).all()


@pytest.mark.parametrize("little", [True, False], ids=["little", "big"])
def test_pfm_both_byte_orders(cvr, tmp_path, little):
    img = picture(7, 5)
    img[0, 0, 0] = np.float32(-2.5)  # a PFM holds any float
    p = tmp_path / "x.pfm"
    p.write_bytes(pfm_bytes(img, little))
    got = cvr.read_image(str(p))
    assert got.shape == (5, 7, 3) and (got.view(np.uint32) == img.view(np.uint32)).all()
    p.write_bytes(pfm_bytes(img, little, scale=2.0))  # the magnitude of the scale line multiplies
    assert (cvr.read_image(str(p)).view(np.uint32) == (img * np.float32(2)).view(np.uint32)).all()


def malformed_files(tmp_path):
    """name -> path of files that are each CVR_ERR_IO."""
    e = rgbe_encode(picture())
    h, w = e.shape[:2]
    flat, rle = hdr_bytes(e, False), hdr_bytes(e, True)
    res = b"-Y %d +X %d\n" % (h, w)
    line = rle_scanline(e[1])
    pfm = pfm_bytes(picture(7, 5), True)
    cases = {
        "empty": b"",
        "two_bytes": b"#?",
        "hdr_truncated_flat": flat[:-1],
        "hdr_truncated_half": flat[:len(flat) // 2],
        "hdr_truncated_rle": rle[:-1],
        "hdr_truncated_rle_mid": rle[:len(HDR_HEAD) + len(res) + 7],
        "hdr_header_only": HDR_HEAD + res,
        "hdr_no_magic": flat[2:],
        "hdr_no_format": b"#?RADIANCE\n\n" + res + e.tobytes(),
        "hdr_other_format": b"#?RADIANCE\nFORMAT=32-bit_rle_xyze\n\n" + res + e.tobytes(),
        "hdr_no_blank_line": b"#?RADIANCE\nFORMAT=32-bit_rle_rgbe\n" + res + e.tobytes(),
        "hdr_other_orientation": HDR_HEAD + b"+Y %d +X %d\n" % (h, w) + e.tobytes(),
        "hdr_resolution_garbage": HDR_HEAD + b"-Y six +X 40\n" + e.tobytes(),
        "hdr_resolution_trailing": HDR_HEAD + b"-Y %d +X %d 3\n" % (h, w) + e.tobytes(),
        "hdr_zero_height": HDR_HEAD + b"-Y 0 +X %d\n" % w + e.tobytes(),
        "hdr_zero_width": HDR_HEAD + b"-Y %d +X 0\n" % h + e.tobytes(),
        "hdr_negative_width": HDR_HEAD + b"-Y %d +X -40\n" % h + e.tobytes(),
        "hdr_huge": HDR_HEAD + b"-Y 65536 +X 65536\n" + e.tobytes(),
        "hdr_overflowing": HDR_HEAD + b"-Y 4294967297 +X 18446744073709551617\n" + e.tobytes(),
        "hdr_endless_header_line": b"#?RADIANCE\n" + b"x" * 5000,
        # a run that passes the scanline's end: 30 + 20 > 40
        "rle_run_past_scanline": HDR_HEAD + b"-Y 1 +X 40\n" + bytes([2, 2, 0, 40, 128 + 30, 7, 128 + 20, 7]) + bytes(64),
        "rle_literal_past_scanline": HDR_HEAD + b"-Y 1 +X 40\n" + bytes([2, 2, 0, 40, 128 + 30, 7, 20]) + bytes(64),
        "rle_zero_count": HDR_HEAD + b"-Y 1 +X 40\n" + bytes([2, 2, 0, 40, 0, 0, 0, 0]) + bytes(64),
        "rle_width_mismatch": HDR_HEAD + b"-Y 1 +X 40\n" + bytes([2, 2, 0, 41]) + line[4:],
        "rle_literal_cut": HDR_HEAD + b"-Y 1 +X 40\n" + bytes([2, 2, 0, 40, 40, 1, 2, 3]),
        "pfm_truncated": pfm[:-1],
        "pfm_header_only": b"PF\n7 5\n-1.0\n",
        "pfm_header_cut": b"PF\n7 5",
        "pfm_grey": b"Pf" + pfm[2:],
        "pfm_zero_width": b"PF\n0 5\n-1.0\n" + pfm[12:],
        "pfm_zero_height": b"PF\n7 0\n-1.0\n" + pfm[12:],
        "pfm_negative": b"PF\n-7 5\n-1.0\n" + pfm[12:],
        "pfm_scale_zero": b"PF\n7 5\n0.0\n" + pfm[12:],
        "pfm_scale_nan": b"PF\n7 5\nnan\n" + pfm[12:],
        "pfm_scale_text": b"PF\n7 5\nfast\n" + pfm[12:],
        "pfm_huge": b"PF\n65536 65536\n-1.0\n" + pfm[12:],
        "not_an_image": b"P6\n7 5\n255\n" + bytes(105),
    }
    paths = {}
    for name, data in cases.items():
        p = tmp_path / (name + ".bin")
        p.write_bytes(data)
        paths[name] = str(p)
    paths["missing"] = str(tmp_path / "no_such_file.hdr")
    return paths


def well_formed_files(tmp_path):
    e = rgbe_encode(picture())
    out = {}
    for name, data in (("flat.hdr", hdr_bytes(e, False)), ("rle.hdr", hdr_bytes(e, True)),
                       ("little.pfm", pfm_bytes(picture(7, 5), True)),
                       ("big.pfm", pfm_bytes(picture(7, 5), False))):
        p = tmp_path / name
        p.write_bytes(data)
        out[name] = str(p)
    return out


def test_malformed_files_are_io_errors(cvr, tmp_path):
    wrong = {}
    for name, path in malformed_files(tmp_path).items():
        try:
            cvr.read_image(path)
            wrong[name] = "read"
        except cvr.CvrError as e:
            if e.code != CVR_ERR_IO:
                wrong[name] = e.code
    assert not wrong, wrong


def test_reader_under_the_host_sanitizers(tmp_path):
    """The stand-alone program (own main, nothing loaded into python) on the same files."""
    exe = tmp_path / "image_io_san"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "image_io_san.cpp"),
                           os.path.join(ROOT, "cudavolumerenderer_amd", "csrc", "cvr_image_io.cpp"), "-o", str(exe)])
    bad, good = malformed_files(tmp_path), well_formed_files(tmp_path)
    names = list(bad) + list(good)
    r = subprocess.run([str(exe)] + [bad[n] for n in bad] + [good[n] for n in good], capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = r.stdout.splitlines()
    assert len(lines) == len(names)
    for name, line in zip(names, lines):
        status = int(line.split()[0])
        assert status == (CVR_ERR_IO if name in bad else 0), (name, line)
    w, h = lines[len(bad)].split()[1:3]
    assert (w, h) == ("40", "6")
