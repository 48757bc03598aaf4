"""Anchors of the SIFT and SURF oracles (oracle/sift.cpp, oracle/surf.cpp) to float64 models of the two
orientation assignments, the 128 and 64 descriptor entries and SIFT's sub-pixel refinement, as functions of the
pixels (sift_reference.py, surf_reference.py: written from Lowe 2004, Bay et al. 2008 and OpenCV's documented
definitions, not from the oracles).  test_detector_anchors.py pins blob position, size, sign and the ramp's
angle to 4 to 9 degrees; nothing there notices a transposed cell grid, reversed orientation bins, 360 - angle
applied twice, a window rotated the wrong way, dx and dy swapped, a wrong layer sigma or the 0.2 clip in the
wrong place, which the oracle and the device would share.  test_gpu_descriptor_anchors.py applies the same
checks to the device.  CPU only.

Tolerances (each stated where it is defined): SIFT descriptor |d - min(v64, 255)| <= 0.5 + EPS, EPS = 0.04;
SIFT angle TOL_DEG = 0.0003; SURF angle 0.3 degrees; SURF descriptor a derived per-entry bound, 4.8e-6 for a
keypoint without uncertain pixels; SIFT refinement first-order bounds from a pyramid error of 2.1e-4 grey.

Measured on the committed oracle (printed by the tests):
  SIFT descriptor  |d - v64| - 0.5 at most 0.0102 (edge_blobs), 0.0039 elsewhere; 19200 entries, 2 above 255.
  SIFT angle       decided keypoints: at most 0.000077 degrees (anchor), 0.000033 elsewhere.  Undecided: anchor 7
                   of 24 (all at the blob centred on a pixel), corner_blobs_96 26 of 40, none elsewhere: 33 of
                   150, under the quarter allowed.  30 of them are within 0.000126 degrees of a variant's peak.
                   Three are not, all at anchor's (50.23, 110.23): angles 31.706, 58.308 and 214.593 degrees,
                   0.0287, 0.0150 and 0.4999 degrees from the nearest variant peak.  These three, named in
                   ANCHOR_SPLIT_OK, are held to Orientation.reachable instead, which at that position accepts
                   36 % of the circle: their angles are in effect not pinned.  No other keypoint, on the CPU
                   or the device, may use that way.  noise_96, block_noise_40, edge_blobs, ridges and
                   ramp_blob_37 have no undecided keypoint, and are asserted so.
                   Outside the cases: noise_176 has one decided keypoint 0.0037 degrees off.
  SIFT refinement  none skipped (condition number <= 100); position, size and response within 0.018 of their
                   bounds, the layer byte within 0.67 of 0.5 + 255 dx.
  SURF angle       at most 0.1041 degrees (noise_96), 0.0096 elsewhere; none excluded.  One keypoint of anchor
                   sits on a centred symmetric blob whose eight equal windows are told apart by rounding
                   only: the oracle's is one of them (WINDOW_TIE); it is the only keypoint matched to a
                   window other than the first largest, which the tests assert.
  SURF descriptor  without uncertain pixels: at most 8.0e-8 (bound 4.8e-6), all keypoints of anchor, the seven
                   ramps and corner_blobs_96, 17 of 112 of noise_96; with: at most 2.4e-3 and 0.958 of the
                   derived bound (ridges); none excluded."""
import numpy as np
import pytest

import detector_cases as dc
import sift_reference as sift_ref
import surf_reference as surf_ref

CASES = ("anchor", "ramp_blob_37", "ramp_blob_270", "ridges", "edge_blobs", "block_noise_40", "corner_blobs_96", "noise_96",
         "surf_blobs_40")
SMOOTH = ("anchor",) + tuple(f"ramp_blob_{a}" for a in dc.RAMP_ANGLES)
SURF_CASES = tuple(dict.fromkeys(CASES + SMOOTH))
NO_UNDECIDED = ("noise_96", "block_noise_40", "edge_blobs", "ridges", "ramp_blob_37")
# (x, y, angle) of the undecided keypoints of anchor that lie outside the three variants' peaks
ANCHOR_SPLIT_OK = ((50.2313, 110.2312, 31.7058), (50.2313, 110.2312, 58.3083), (50.2313, 110.2312, 214.5928))
_RUN = {}


def _case(name):
    return next(c for c in dc.cases() if c.name == name)


def split_ok(name):
    return ANCHOR_SPLIT_OK if name == "anchor" else ()


def _sift(oracle_mod, name):
    """check_features on the oracle's SIFT output of a case, run once: its figures, or the error it raised."""
    if name not in _RUN:
        img = _case(name).img
        kps, desc = oracle_mod.sift_detect_and_compute(img)
        try:
            _RUN[name] = sift_ref.check_features(img, kps, desc, f"oracle SIFT {name}", split_ok=split_ok(name))
        except AssertionError as e:
            _RUN[name] = e
    if isinstance(_RUN[name], AssertionError):
        raise _RUN[name]
    return _RUN[name]


@pytest.mark.parametrize("name", CASES)
def test_sift_against_float64(oracle_mod, name):
    got = _sift(oracle_mod, name)
    assert got["checked"] >= _case(name).min_sift
    if name in NO_UNDECIDED:
        assert got["undecided"] == 0
    assert len(got["by_split"]) == (3 if name == "anchor" else 0)


def test_fast_atan2_is_atan2_to_a_hundredth_of_a_degree():
    """The model's sample angles are the published polynomial's; this ties them to atan2 (measured 0.009547)."""
    assert sift_ref.fast_atan2_error() < 0.01


def test_reachable_accepts_the_variants_peaks_and_rejects_a_far_angle(oracle_mod):
    """Orientation.reachable on its own: every peak of every variant is reachable, at an undecided position
    (anchor's pixel-centred blob) and at a decided one (ramp_blob_37); at the decided one, whose tie weights
    are too small to move a peak, an angle 5 degrees from the only peak is not, nor is the opposite one."""
    for name, want_decided in (("anchor", False), ("ramp_blob_37", True)):
        img = _case(name).img
        kps, _ = oracle_mod.sift_detect_and_compute(img)
        kp = kps[6] if name == "anchor" else kps[0]
        octave, layer, _, _, px, py, s = sift_ref.unpack(kp)
        m = sift_ref.Orientation(sift_ref.ScaleSpace(img).level(octave, layer), px, py, s)
        assert m.decided == want_decided
        for v in m.variants:
            assert len(v) > 0 and all(m.reachable(float(p), sift_ref.TOL_DEG) for p in v)
        if want_decided:
            peak = float(m.variants[0][0])
            assert not m.reachable((peak + 5.0) % 360.0, sift_ref.TOL_DEG)
            assert not m.reachable((peak + 180.0) % 360.0, sift_ref.TOL_DEG)


def test_sift_cases_reach_octaves_layers_saturation_and_cut_windows(oracle_mod):
    runs = [_sift(oracle_mod, n) for n in CASES]
    assert set().union(*(r["octaves"] for r in runs)) >= {-1, 0, 1}
    assert set().union(*(r["layers"] for r in runs)) == {1, 2, 3}
    assert oracle_mod.sift_census(_case("edge_blobs").img)["saturate_255"] > 0 and _sift(oracle_mod, "edge_blobs")["saturated"] > 0
    cut = oracle_mod.sift_census(_case("corner_blobs_96").img)
    assert cut["orientation_window_cut"] > 0 and cut["descriptor_samples_skipped"] > 0
    assert oracle_mod.surf_census(_case("corner_blobs_96").img)["window_samples_clamped"] > 0


def test_sift_undecided_share(oracle_mod):
    """Undecided keypoints plus those the refinement check skips: at most a quarter of all keypoints of the
    cases.  Measured 33 + 0 of 150."""
    runs = [_sift(oracle_mod, n) for n in CASES]
    left, total = sum(r["undecided"] + r["skipped"] for r in runs), sum(r["checked"] for r in runs)
    print(f"SIFT: {left} of {total} keypoints undecided or skipped")
    assert 4 * left <= total, (left, total)


@pytest.mark.parametrize("name", SURF_CASES)
def test_surf_against_float64(oracle_mod, name):
    c = _case(name)
    for thr in sorted({400.0, c.surf_thr}):
        kps, desc = oracle_mod.surf_detect_and_compute(c.img, thr)
        if c.min_surf == 0 and len(kps) == 0:
            continue  # the 40 x 30 cases made for SIFT have no SURF keypoint
        got = surf_ref.check_features(c.img, kps, desc, f"oracle SURF {name} at {thr}", smooth=name in SMOOTH)
        assert got["other_window"] == (1 if name == "anchor" else 0)
        assert got["checked"] >= (c.min_surf if thr == c.surf_thr else 1)


# Negative controls: the checks fail on the oracle's own output altered in the ways they are there to notice.

@pytest.fixture(scope="module")
def sift_noise(oracle_mod):
    img = _case("noise_96").img
    return (img,) + oracle_mod.sift_detect_and_compute(img)


@pytest.fixture(scope="module")
def surf_noise(oracle_mod):
    img = _case("noise_96").img
    return (img,) + oracle_mod.surf_detect_and_compute(img, 400.0)


def _with_angle(kps, angle):
    out = kps.copy()
    out["angle"] = angle
    return out


def test_sift_control_cell_grid_transposed(sift_noise):
    img, kps, desc = sift_noise
    bad = np.ascontiguousarray(desc.reshape(-1, 4, 4, 8).transpose(0, 2, 1, 3)).reshape(-1, 128)
    with pytest.raises(AssertionError, match="descriptor"):
        sift_ref.check_features(img, kps, bad, "control: cell grid transposed")


def test_sift_control_orientation_bins_reversed(sift_noise):
    img, kps, desc = sift_noise
    bad = np.ascontiguousarray(desc.reshape(-1, 16, 8)[:, :, ::-1]).reshape(-1, 128)
    with pytest.raises(AssertionError, match="descriptor"):
        sift_ref.check_features(img, kps, bad, "control: orientation bins reversed")


def test_sift_control_descriptor_for_kp_angle(sift_noise):
    """The oracle's descriptors handed over with keypoints whose angle is negated: what a descriptor computed
    for kp.angle instead of 360 - kp.angle looks like to the check."""
    img, kps, desc = sift_noise
    with pytest.raises(AssertionError, match="descriptor"):
        sift_ref.check_features(img, _with_angle(kps, (360.0 - kps["angle"]) % 360.0), desc, "control: angle negated")


def test_sift_control_angle_shifted_10_degrees(sift_noise):
    img, kps, desc = sift_noise
    with pytest.raises(AssertionError, match="'angle"):
        sift_ref.check_features(img, _with_angle(kps, (kps["angle"] + 10.0) % 360.0), desc, "control: angle + 10")


def test_sift_control_base_sigma_1_5(sift_noise):
    """The model's pyramid built with sigma 1.5: the oracle's output must not fit it."""
    img, kps, desc = sift_noise
    with pytest.raises(AssertionError):
        sift_ref.check_features(img, kps, desc, "control: model sigma 1.5", base_sigma=1.5)


def test_sift_control_offset_mirrored(sift_noise):
    """The stored position mirrored about the level pixel (x = -H^-1 g with the wrong sign): descriptor and
    orientation read the same pixel, the refinement check fails."""
    img, kps, desc = sift_noise
    bad = kps.copy()
    for f in ("x", "y"):
        scale = np.array([sift_ref.unpack(k)[3] for k in kps])
        level = kps[f].astype(np.float64) * scale
        bad[f] = ((2.0 * np.rint(level) - level) / scale).astype(np.float32)
    with pytest.raises(AssertionError, match="refinement"):
        sift_ref.check_features(img, bad, desc, "control: offset mirrored")


def test_surf_control_dx_dy_swapped(surf_noise):
    img, kps, desc = surf_noise
    bad = np.ascontiguousarray(desc.reshape(-1, 16, 4)[:, :, [1, 0, 3, 2]]).reshape(-1, 64)
    with pytest.raises(AssertionError, match="descriptor"):
        surf_ref.check_features(img, kps, bad, "control: dx and dy swapped", max_keypoints=32)


def test_surf_control_dx_sign_flipped(surf_noise):
    img, kps, desc = surf_noise
    bad = desc.reshape(-1, 16, 4).copy()
    bad[:, :, 0] *= -1.0
    with pytest.raises(AssertionError, match="descriptor"):
        surf_ref.check_features(img, kps, bad.reshape(-1, 64), "control: dx sign flipped", max_keypoints=32)


def test_surf_control_angle_mirrored(surf_noise):
    img, kps, desc = surf_noise
    with pytest.raises(AssertionError, match="'angle"):
        surf_ref.check_features(img, _with_angle(kps, (360.0 - kps["angle"]) % 360.0), desc, "control: angle mirrored",
                                max_keypoints=32)


def test_surf_control_cell_grid_transposed(surf_noise):
    img, kps, desc = surf_noise
    bad = np.ascontiguousarray(desc.reshape(-1, 4, 4, 4).transpose(0, 2, 1, 3)).reshape(-1, 64)
    with pytest.raises(AssertionError, match="descriptor"):
        surf_ref.check_features(img, kps, bad, "control: cell grid transposed", max_keypoints=32)
