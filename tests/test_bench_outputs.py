"""bench.py's plain run and --dump-outputs: a plain run prints the headline line alone
(everything that takes runs of its own is behind --full), and --dump-outputs DIR leaves
the last timed step's host image in DIR/image.npy and DIR/image_nonfinite.npy (finite
numbers only: NaN pixels are marked in the second file): the same image a caller of
cvr_render_image receives, within the fp32 summation-order bound.  An image above the
size limit is written as a fixed, seeded sample of its pixels."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from parity_util import assert_pixels_close

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402

FULL_ONLY = ("roofline", "cpu_baseline", "serial", "shard_emulation", "ranks", "weak")


def _load_dump(d):
    """(image, kinds) of a dump; every file of it is float32 or float64 and finite."""
    for f in os.listdir(d):
        a = np.load(os.path.join(d, f))
        assert a.dtype in (np.float32, np.float64) and np.isfinite(a).all(), f
    return np.load(os.path.join(d, "image.npy")), np.load(os.path.join(d, "image_nonfinite.npy"))


def _restore(img, kind):
    out = img.copy()
    for k, v in ((1, np.nan), (2, np.inf), (3, -np.inf)):
        out[kind == k] = v
    return out


def test_dump_outputs_small_image_is_written_whole(tmp_path):
    img = np.random.default_rng(1).random((5, 7, 4), dtype=np.float32)
    img[2, 3, 0], img[0, 1, 2], img[4, 6, 3] = np.nan, np.inf, -np.inf  # part of the output, written as kinds
    bench.dump_outputs(str(tmp_path / "d"), img)
    assert sorted(os.listdir(tmp_path / "d")) == ["image.npy", "image_nonfinite.npy"]
    got, kind = _load_dump(tmp_path / "d")
    assert np.flatnonzero(kind).tolist() == np.flatnonzero(~np.isfinite(img)).tolist()
    assert (kind[2, 3, 0], kind[0, 1, 2], kind[4, 6, 3]) == (1, 2, 3)
    assert got.shape == img.shape and (got[kind != 0] == 0).all()
    assert (got.view(np.uint32) == img.view(np.uint32))[kind == 0].all()
    assert (_restore(got, kind).view(np.uint32) == img.view(np.uint32)).all()


def test_dump_outputs_large_image_is_a_fixed_sample(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_MAX_BYTES", 4096)
    img = np.arange(64 * 48 * 4, dtype=np.float32).reshape(48, 64, 4)  # 48 KiB
    bench.dump_outputs(str(tmp_path / "a"), img)
    bench.dump_outputs(str(tmp_path / "b"), img + 1)
    (px, kind), idx = _load_dump(tmp_path / "a"), np.load(tmp_path / "a" / "image_pixel_index.npy")
    assert px.dtype == np.float32 and idx.dtype == np.float64 and not kind.any()
    assert px.nbytes + kind.nbytes + idx.nbytes <= 4096 and px.shape == kind.shape == (len(idx), 4) and len(idx) > 64
    i = idx.astype(np.int64)
    assert (np.diff(i) > 0).all() and i[0] >= 0 and i[-1] < 48 * 64
    assert (px == img.reshape(-1, 4)[i]).all()
    # the same pixels whatever the image holds: two builds' dumps compare pixel for pixel
    assert (np.load(tmp_path / "b" / "image_pixel_index.npy") == idx).all()
    assert (np.load(tmp_path / "b" / "image.npy") == px + 1).all()


@pytest.mark.gpu
def test_plain_run_prints_the_headline_and_dumps_the_image(cvr, tmp_path):
    W, H, iters, steps = 160, 96, 3, 3
    out = tmp_path / "out"
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps),
                        "--warmup", "1", "--resolution", str(W), str(H), "--iterations", str(iters),
                        "--dump-outputs", str(out)], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stderr[-2000:]
    js = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(js) == 1, r.stdout[-2000:]
    line = json.loads(js[0])
    assert not [k for k in FULL_ONLY if k in line], sorted(line)
    assert line["steps"] == steps and line["unit"] == "Msamples/s" and line["dtype"] == "f32"
    assert line["higher_is_better"] is True and line["metric"] == bench.METRIC
    assert line["ms_per_step"] > 0
    # value is the workload's samples over one step's time (both rounded in the line)
    assert line["value"] == pytest.approx(W * H * iters / (line["ms_per_step"] * 1e-3) / 1e6, rel=1e-2)
    assert sorted(os.listdir(out)) == ["image.npy", "image_nonfinite.npy"]
    img = _restore(*_load_dump(out))
    assert img.dtype == np.float32 and img.shape == (H, W, 4)
    scene = cvr.Scene.synthetic("manix")
    ctx = cvr.Context(0, "regenerationSK")
    ctx.set_medium(scene.medium)
    iv, r2v = cvr.default_camera(W, H)
    ctx.set_camera(iv, r2v, (W, H))
    ctx.init()
    ref, _ = ctx.render_image(W, H, (1, 1), iters)
    ctx.close()
    assert np.nanmax(ref[..., :3]) > 0
    assert_pixels_close(img[..., :3], ref[..., :3], iters, "bench.py --dump-outputs vs cvr_render_image")
    assert line["nan_pixels"] == int(np.isnan(ref[..., :3]).any(-1).sum())
