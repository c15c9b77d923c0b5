"""bench.py's plain run and its --full / --dump-outputs options.

CPU: the option defaults, --steps validation and the dump writer (float32,
whole frame or a fixed seeded sample under the 64 MB limit).  GPU: a plain
run of a small frame times exactly --steps steps, carries the headline fields
and none of the --full measurements, and dumps the frame a direct render of
the same parameters gives; a --full run of the same frame adds them."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import REPO

sys.path.insert(0, REPO)

HEADLINE = {"metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step", "steps", "warmup", "n_gpus"}
FULL_ONLY = {"roofline", "f32_hybrid_variant", "wavefront_variant", "globe_10k_variant", "cornell_variant",
             "cpu_baseline"}
SMALL = ("--width", "160", "--spp", "8")  # 160x90 at 8 spp: more than one block, a fraction of a second


def test_full_and_dump_are_off_by_default():
    import bench
    a = bench.parse_args(["--gpus", "1", "--steps", "7", "--warmup", "3"])
    assert (a.full, a.dump_outputs, a.steps, a.warmup) == (False, None, 7, 3)
    a = bench.parse_args(["--full", "--dump-outputs", "somewhere"])
    assert a.full is True and a.dump_outputs == "somewhere"
    with pytest.raises(SystemExit):
        bench.parse_args(["--steps", "0"])


def test_dump_writes_the_whole_frame_as_float32(tmp_path):
    import bench
    import torch
    frame = torch.arange(90 * 160 * 3, dtype=torch.int64).remainder(251).to(torch.uint8).reshape(90, 160, 3)
    bench.dump_outputs(str(tmp_path / "d"), frame)
    assert os.listdir(tmp_path / "d") == ["image.npy"]
    img = np.load(tmp_path / "d" / "image.npy")
    assert img.dtype == np.float32 and img.shape == (90, 160, 3)
    assert np.array_equal(img, frame.numpy().astype(np.float32))


def test_dump_samples_a_frame_over_the_limit(tmp_path, monkeypatch):
    """Over the limit: the same seeded pixel sample on every run, values and
    indices together under the limit (configs[2]'s 3840x2160 frame: 40 MB)."""
    import bench
    import torch
    assert bench.DUMP_LIMIT_BYTES + 2 * 128 <= 64_000_000  # (two .npy headers of 128 bytes)
    assert bench.DUMP_SAMPLE_PIXELS * (3 * 4 + 8) <= bench.DUMP_LIMIT_BYTES
    monkeypatch.setattr(bench, "DUMP_LIMIT_BYTES", 4096)  # the same path at a test-sized frame
    monkeypatch.setattr(bench, "DUMP_SAMPLE_PIXELS", 100)
    frame = torch.arange(40 * 30 * 3, dtype=torch.int64).remainder(251).to(torch.uint8).reshape(40, 30, 3)
    got = []
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), frame)
        got.append((np.load(tmp_path / d / "image.npy"), np.load(tmp_path / d / "image_index.npy")))
    (img, idx), (img2, idx2) = got
    assert np.array_equal(idx, idx2) and np.array_equal(img, img2)
    assert img.dtype == np.float32 and img.shape == (100, 3) and idx.dtype == np.float64 and idx.shape == (100,)
    assert np.all(np.diff(idx) > 0) and idx[0] >= 0 and idx[-1] < 40 * 30
    assert np.array_equal(img, frame.numpy().reshape(-1, 3)[idx.astype(np.int64)].astype(np.float32))
    assert img.nbytes + idx.nbytes <= 4096


def run_bench(*argv):
    p = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "1", *argv], capture_output=True,
                       text=True, timeout=120, cwd=REPO)
    assert p.returncode == 0, p.stderr[-4000:]
    lines = [l for l in p.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, p.stdout
    return json.loads(lines[0])


@pytest.fixture(scope="module")
def plain(tmp_path_factory):
    """One plain run, shared: (its line, its dump directory)."""
    out = tmp_path_factory.mktemp("plain") / "dump"
    return run_bench("--steps", "3", "--warmup", "1", *SMALL, "--dump-outputs", str(out)), out


@pytest.mark.gpu
def test_plain_run_is_the_headline_only_and_dumps_the_frame(rtw, plain):
    import torch
    from rtw_amd.device import TorchRenderer
    r, out = plain
    assert HEADLINE <= set(r) and not FULL_ONLY & set(r) and r["full"] is False
    assert (r["steps"], r["warmup"], r["unit"], r["higher_is_better"], r["dtype"]) == (3, 1, "Msamples/s", True, "f64")
    assert r["metric"].startswith("Msamples/sec")
    assert len(r["dist"]["rank_step_ms"]) == 1 and r["ms_per_step"] > 0
    # value = the frame's samples over one timed step, within rounding
    samples = 160 * 90 * 8
    assert abs(r["value"] - samples / (r["ms_per_step"] * 1e-3) / 1e6) <= 0.01 * r["value"] + 0.01
    assert sorted(os.listdir(out)) == ["image.npy"]
    img = np.load(out / "image.npy")
    assert img.dtype == np.float32 and img.shape == (90, 160, 3)
    sph, mats, _ = rtw.cover_scene(42)
    ref = TorchRenderer(sph, mats, 0).render(rtw.cover_camera(16 / 9), rtw.make_params(160, 90, 8, 50, 42))
    torch.cuda.synchronize()
    assert np.array_equal(img, ref.cpu().numpy().astype(np.float32))


@pytest.mark.gpu
def test_full_run_adds_the_roofline_and_the_variants(plain, tmp_path):
    out = tmp_path / "dump"
    r = run_bench("--full", "--steps", "2", "--warmup", "1", *SMALL, "--no-cpu-baseline", "--no-world-variants",
                  "--dump-outputs", str(out))
    assert HEADLINE <= set(r) and r["full"] is True and r["steps"] == 2
    assert {"roofline", "f32_hybrid_variant", "wavefront_variant"} <= set(r)
    roof = r["roofline"]
    assert roof["kernel"] == "trace_kernel" and roof["flop_per_launch"] > 0 and roof["sclk_mhz"] > 0
    # the dump is the headline's last timed frame (f64), not a variant's that rendered after it
    assert np.array_equal(np.load(out / "image.npy"), np.load(plain[1] / "image.npy"))
