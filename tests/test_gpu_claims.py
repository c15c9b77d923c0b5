"""The megakernel's guided claims (csrc/rtw_claim.hpp): a wave of the primary-first loop in a run
of proven-empty batches claims several 64-unit batches of the queue with one atomic, keeps them as its
reserve, and reuses a tile's beam pass for the tile's further batches.  Every frame is bit-identical (max|d| = 0) to oracle Tier B, the counting
pass's samples, segments and sphere tests are the oracle's, the units finished without tracing are the HOST
rule's (tests/sky_helpers.py) and the mask popcount — counted per fetched batch, its pass made or reused — is
the host evaluation of csrc/rtw_beam.hpp times the chunks; the f64 chunk sums themselves are compared with
the masked kernel's (the rotated loop, which claims one batch at a time).

A claim is larger than one batch only in a run of proven-empty batches and while more than 2 x kClaimDiv
batches per wave of the grid are left (claim_k, guided_k), and a grid has a wave per batch up to the device's resident
waves; a launch whose queue is too short for a claim of two runs without the reserve (TraceArgs::claim_waves 0):
the small frames below hold that path to the same frames, counts and popcounts, the queue's end included,
and the four frames of more than 32,768 batches (one-sample and two-sample units, so they stay a few million
samples) run the larger claims, down to one.  Claim counts vary from run to run: they are bounded, not pinned.

The last-first unit order is a development knob (RTW_UNIT_ORDER=rev, -DRTW_MEASURE builds only):
test_last_first_unit_order runs this file once more in a child process with the development library
(lib_m/librtw_hip.so, which `make` builds next to the product library) and that knob; every frame, count and
popcount assertion holds in that order too, with cameras turned so that the proven tiles lead the dealt queue
(REV below).  tests/test_claim_host.py simulates both orders."""
import os
import subprocess
import sys

import numpy as np
import pytest

from helpers import host_masks, to_oracle_scene
from sky_helpers import gpu_check

pytestmark = pytest.mark.gpu

ASPECT = 16 / 9
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MEASURE_LIB = os.path.join(REPO, "raytracinginoneweekend.zig_amd", "lib_m", "librtw_hip.so")
REV = os.environ.get("RTW_UNIT_ORDER") == "rev"  # this process is test_last_first_unit_order's child


@pytest.fixture(scope="module")
def cover(rtw, oracle):
    from rtw_amd.device import TorchRenderer
    sph, mats, _ = rtw.cover_scene(42)
    return sph, to_oracle_scene(oracle, sph, mats), TorchRenderer(sph, mats, 0), rtw.cover_camera(ASPECT)


def up_camera(rtw):
    """The cover camera turned upwards: only background."""
    return rtw.camera_init((13, 2, 3), (13, 12, 3), (0, 0, 1), 20.0, ASPECT, 0.1, 10.0, 0.0, 1.0)


def raised_camera(rtw):
    """The cover camera aimed 3 higher: the sky fills the upper 11 of a 48x24 frame's 18 tiles and the upper 3
    of a 24x16 frame's 6.  Last-first (REV) the camera is upside down: the sky fills the last tiles of the
    frame (9 of 18, 3 of 6), which lead that order's queue."""
    return rtw.camera_init((13, 2, 3), (0, 3, 0), (0, -1 if REV else 1, 0), 20.0, ASPECT, 0.1, 10.0, 0.0, 1.0)


def rolled_camera(rtw):
    """The cover camera rolled by a quarter turn: the horizon is vertical, so every tile row of the frame
    runs from traced tiles into proven-empty ones (or back) within one claim."""
    return rtw.camera_init((13, 2, 3), (0, 0, 0), (1, 0, -13 / 3), 20.0, ASPECT, 0.1, 10.0, 0.0, 1.0)


def claims_check(rtw, oracle, cover, what, cam=None, **kw):
    """sky_helpers.gpu_check, then the popcount and the bounds every launch's claims and passes obey.
    Returns (stats, batches, tiles, empty tiles)."""
    sph, osc, rend, cover_cam = cover
    cam = cam or cover_cam
    _, st, empty = gpu_check(rtw, oracle, rend, sph, osc, cam, what, **kw)
    p = rtw.make_params(**kw)
    n_chunks = -(-p.spp // min(p.chunk or rtw.DEFAULT_CHUNK, p.spp))
    tiles = -(-p.width // 8) * -(-p.row_count // 8)
    batches = tiles * n_chunks
    print(what, {k: st[k] for k in ("queue_claims", "beam_passes", "primary_mask_popcount", "tail_helped_samples")},
          "batches", batches, "tiles", tiles)
    assert st["primary_rounds"] > 0 or st["untraced_samples"] == st["samples"] or p.max_depth == 0, st
    assert st["primary_mask_popcount"] == n_chunks * host_masks(sph, cam, p)["popcount"], (what, st)
    # one atomic fetches at least one batch and at most kClaimMax (8); every wave's last claim lies past the end
    assert st["queue_claims"] >= -(-batches // 8) + 1, (what, st, batches)
    # a pass per claim's first batch at the most, and one per tile change along the queue (tiles - 1)
    assert 1 <= st["beam_passes"] <= st["queue_claims"] + tiles - 1, (what, st, tiles)
    return st, batches, tiles, empty


SMALL = [
    ("64x36, 1 chunk: every batch another tile", dict(width=64, height=36, spp=7, chunk=7)),
    ("64x36, 2 chunks", dict(width=64, height=36, spp=8, chunk=4)),
    ("64x36, 5 chunks", dict(width=64, height=36, spp=10, chunk=2)),
    ("64x36, 7 chunks", dict(width=64, height=36, spp=7, chunk=1)),
    ("100x37: padding tiles, 5 chunks", dict(width=100, height=37, spp=10, chunk=2)),
    ("rows 1::3 of 384x216, 2 chunks", dict(width=384, height=216, spp=4, chunk=2, row_begin=1, row_stride=3)),
    ("16x8: two batches for four waves, two first claims past the end", dict(width=16, height=8, spp=4)),
    ("8x8: one batch", dict(width=8, height=8, spp=6, chunk=4)),
    ("128x72 max_depth 0", dict(width=128, height=72, spp=7, chunk=3, max_depth=0)),
    ("128x72 max_depth 1", dict(width=128, height=72, spp=7, chunk=3, max_depth=1)),
]


@pytest.mark.parametrize("what,kw", SMALL, ids=[s[0].split(":")[0] for s in SMALL])
def test_small_frames(rtw, oracle, cover, what, kw):
    claims_check(rtw, oracle, cover, what, **kw)


def test_camera_turned_up_small(rtw, oracle, cover):
    st, batches, _, empty = claims_check(rtw, oracle, cover, "up, 100x50", cam=up_camera(rtw), width=100, height=50, spp=7,
                                         chunk=3, background=(0.1, 0.7, 1 / 3))
    assert len(empty) == 13 * 7 and st["untraced_samples"] == st["samples"] == 100 * 50 * 7


def test_long_queue_claims_several_batches(rtw, oracle, cover):
    """The raised camera, 48x24 at 4,096 samples in chunks of 2: 18 tiles x 2,048 chunks = 36,864 batches, a
    tile's chunks in a row, the 11 proven tiles first.  Fewer atomics than batches, a beam pass per claim at
    the most, and the tail still deals."""
    st, batches, tiles, empty = claims_check(rtw, oracle, cover, "raised, 48x24x4096 chunk 2", cam=raised_camera(rtw), width=48,
                                             height=24, spp=4096, chunk=2)
    assert batches == 36864 >= 2000 and len(empty) == (9 if REV else 11)
    # (last-first only 8 proven tiles lead the queue, 16,384 batches: the atomics they save are about the
    # 4,096 claims past the end, so that order's bound is the next test's)
    if not REV:
        assert st["queue_claims"] < batches, st
    assert st["beam_passes"] <= st["queue_claims"] + (tiles - 1), st
    assert st["tail_helped_samples"] > 0, st


def test_long_queue_traced_tile_reuses_its_pass(rtw, oracle, cover):
    """The raised camera, 24x16 at 8,192 one-sample chunks: 6 tiles x 8,192 chunks = 49,152 batches, the 3
    proven tiles first in both unit orders.  When the run of proven batches ends, 24,576 batches are left, the
    guided K is 3, and the claims made in the run reach into the first traced tile: its batches that wait in
    a reserve reuse the pass of the first of them, with a mask that is not empty.  The popcount is still the
    host's per fetched batch (claims_check), which it would not be if it were added per beam pass."""
    st, batches, tiles, empty = claims_check(rtw, oracle, cover, "raised, 24x16x8192 chunk 1", cam=raised_camera(rtw), width=24,
                                             height=16, spp=8192, chunk=1)
    assert batches == 49152 and empty == ([3, 4, 5] if REV else [0, 1, 2])
    assert st["primary_mask_popcount"] > 0
    assert st["queue_claims"] < batches, st
    assert st["beam_passes"] < batches, st


def test_long_queue_whole_claims_empty(rtw, oracle, cover):
    """The camera turned up, 64x36 at 1,024 one-sample chunks: 40,960 batches, every claim proven empty from
    one pass, no closest hit."""
    st, batches, _, empty = claims_check(rtw, oracle, cover, "up, 64x36x1024 chunk 1", cam=up_camera(rtw), width=64, height=36,
                                         spp=1024, chunk=1, background=(0.1, 0.7, 1 / 3))
    assert batches == 40960 and len(empty) == 40
    assert st["untraced_units"] == 64 * 36 * 1024 and st["primary_rounds"] == 0 and st["sphere_loop_wave_iters"] == 0
    assert st["queue_claims"] < batches and st["beam_passes"] <= st["queue_claims"] + 39, st


def test_long_queue_empty_and_traced_tiles_in_one_claim(rtw, oracle, cover):
    """The rolled camera, 2048x1152 at one sample: 36,864 tiles of one chunk each, so every batch of a claim is
    another tile and the claims made in a tile row's empty part reach into its traced part."""
    kw = dict(width=2048, height=1152, spp=1, max_depth=2)
    st, batches, tiles, empty = claims_check(rtw, oracle, cover, "rolled, 2048x1152x1", cam=rolled_camera(rtw), **kw)
    assert batches == tiles == 36864
    assert 0.1 * tiles < len(empty) < 0.9 * tiles, len(empty)
    es = set(empty)
    assert sum(1 for t in empty if (t + 1) % 256 and (t + 1) not in es) > 100  # tile rows that change sides
    assert st["beam_passes"] == batches, st  # one chunk: nothing to reuse


def test_f64_sums_are_the_masked_kernels(rtw, cover):
    """The f64 chunk sums, which 8-bit pixels round away: a pass of 128x72 at 20 samples in one chunk (claims
    of one batch, 9 proven tiles) and one of 48x24 at 4,096 samples in chunks of 2 from the raised camera
    (36,864 batches, claims of up to four) against the same passes through the masked kernel on all pixels but one."""
    import torch
    from rtw_amd.device import TorchAccumulator
    _, _, rend, cover_cam = cover
    for cam, kw, n in ((cover_cam, dict(width=128, height=72, spp=20, chunk=20), 20),
                       (raised_camera(rtw), dict(width=48, height=24, spp=4096, chunk=2), 4096)):
        p = rtw.make_params(background=(0.1, 0.7, 1 / 3), **kw)
        a = TorchAccumulator(rend.scene, p)
        a.render_pass(cam, n)
        torch.cuda.synchronize()
        sa, _ = a.read()
        a.close()
        mask = np.ones((kw["height"], kw["width"]), np.uint8)
        mask[-1, -1] = 0
        b = TorchAccumulator(rend.scene, p)
        b.set_mask(mask)
        b.render_pass(cam, n)
        torch.cuda.synchronize()
        sb, _ = b.read()
        b.close()
        assert (sa[mask != 0] > 0).any()
        assert np.array_equal(sb[mask != 0], sa[mask != 0]), kw


def test_development_library_reads_the_knobs(rtw, cover):
    """In the child process of the next test: the library is the -DRTW_MEASURE build, whose counting pass
    takes RTW_PHASE_PROFILE (the product library refuses it), so RTW_UNIT_ORDER=rev is read too."""
    if not REV:
        return
    _, _, rend, cam = cover
    os.environ["RTW_PHASE_PROFILE"] = "1"
    try:
        rend.stats(cam, rtw.make_params(width=16, height=8, spp=4))
    finally:
        del os.environ["RTW_PHASE_PROFILE"]


@pytest.mark.skipif(REV, reason="this process is the child")
@pytest.mark.skipif(not os.path.exists(MEASURE_LIB), reason="no development library (make lib_m/librtw_hip.so)")
def test_last_first_unit_order():
    """Every test of this file in a child process with the development library and RTW_UNIT_ORDER=rev."""
    env = dict(os.environ, RTW_LIB_PATH=MEASURE_LIB, RTW_UNIT_ORDER="rev")
    p = subprocess.run([sys.executable, "-m", "pytest", "-q", "-s", "-p", "no:cacheprovider", os.path.abspath(__file__)],
                       env=env, cwd=REPO, capture_output=True, text=True, timeout=600)
    print(p.stdout[-6000:])
    assert p.returncode == 0 and " passed" in p.stdout and "failed" not in p.stdout, p.stdout[-3000:] + p.stderr[-2000:]
