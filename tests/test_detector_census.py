"""Which branches of SIFT and SURF the detector cases (detector_cases.py) enter, counted by the oracle
(oracle.sift_census / surf_census: counters inside oracle/sift.cpp and oracle/surf.cpp) and asserted, as
test_oracle_kats.py::test_ransac_hypothesis_sets_reach_their_regimes does for RANSAC.  The GPU kernels
follow the oracle branch for branch (csrc/sift.hip refine_body / sort_body / descriptor_body, csrc/surf.hip),
and test_gpu_detector_regimes.py compares them with the oracle on these cases: a counter above zero here
is a device branch that test executes.  CPU only.

Branches no input reached (UNREACHED; only counters of the closed *_MAY_BE_UNREACHED lists may stand there,
anything else that cannot be reached is a finding to report):

saturate_255, which may be unreached, is reached: not by a blob whose descriptor window lies mostly outside a
40 x 30 frame (5 such blobs and 1500 random ones: 0) but by a blob beside a sharp step edge (edge_blobs: the
edge's few gradient bins hold over 84 % of the descriptor's energy, 2 values above 255).

SIFT
  reject_int_max_3 an offset above INT_MAX / 3 needs a 3 x 3 determinant some nine orders of magnitude
                    below its cofactors that is not exactly 0.  Tried: the ridges case (exactly 0: d_eq_0) and
                    300 copies of it with 1 to 40 pixels moved by one grey level (1451 more d_eq_0, no huge offset).
  snap_to_0         the interpolated peak must be bin 0 to within 1.5e-6 of a bin: hist[35] == hist[1] to 6
                    digits.  Tried: ramps at angle 0 (slopes 1, 2.5, 4) under blobs and blob pairs mirror-symmetric
                    about a horizontal axis on a row, between two rows and at the quarter rows (360 scenes, 662
                    keypoints), and the orientation anchor of angle 0.  The 2x upscale puts the axis of a symmetric
                    image a quarter pixel off every row of every octave, so the two bins never agree exactly.
  o0_ge_n           needs a sample of gradient angle 360 (dy < 0 below dx by 7 digits) at a keypoint of angle 0
                    to within 1.5e-5 degrees, that is snap_to_0 first.  Tried: the same scenes.
SURF
  d_eq_0            the diagonal of the 3 x 3 system is strictly negative at a strict maximum (each of a00, a11,
                    a22 is a sum that cannot round to 0), so d == 0 needs an exact cancellation between float
                    products; not structural, never seen (5020 maxima here, 1866 of them exact ties of the response).
  reject_all_zero   needs d == 0, or a zero right-hand side: det equal left and right, above and below AND in the
                    layers below and above the maximum; mirror-symmetric images give the first two, nothing the third.
  drop_gws          gws = 2 round(2 s), s = 1.2 size / 9, is at most 0.54 size + 1.  A layer has samples to scan
                    only if rows > 2 margin, that is if the layer above it is smaller than min(w, h), and
                    interpolation moves size by at most one layer step, up to that layer's: gws < min(sw, sh), dead code.
  drop_nang         the disc's centre sample (offset 0, 0) is at round(kp - (gws - 1) / 2) with kp at least
                    margin * step from each border and gws / 2 < margin * step, so it is inside: nang >= 1, dead code.
  class_id_0        trace == 0 is dx == -dy, det = -dx^2 - 0.81 dxy^2 <= 0, which fails det > thr >= 0: dead code.
"""
import numpy as np

import detector_cases as dc

SIFT_UNREACHED = ("reject_int_max_3", "snap_to_0", "o0_ge_n")
SURF_UNREACHED = ("d_eq_0", "reject_all_zero", "drop_gws", "drop_nang", "class_id_0")
# the closed lists: what may be left unreached at all
SIFT_MAY_BE_UNREACHED = ("reject_int_max_3", "snap_to_0", "o0_ge_n", "saturate_255")
SURF_MAY_BE_UNREACHED = ("d_eq_0", "reject_all_zero", "drop_gws", "drop_nang", "class_id_0")

_CENSUS = None


def census(oracle_mod):
    """Once per session: per case (SIFT census, SURF census summed over thresholds 400 and the case's,
    SIFT keypoints, SURF keypoints at the case's threshold)."""
    global _CENSUS
    if _CENSUS is None:
        out = []
        for c in dc.cases():
            s = oracle_mod.sift_census(c.img)
            ks, _ = oracle_mod.sift_detect_and_compute(c.img)
            u = oracle_mod.surf_census(c.img, 400.0)
            for k, v in oracle_mod.surf_census(c.img, c.surf_thr).items():
                u[k] += v
            ku, _ = oracle_mod.surf_detect_and_compute(c.img, c.surf_thr)
            out.append((c, s, u, ks, ku))
        _CENSUS = out
    return _CENSUS


def _table(title, names, rows):
    print(f"\n{title}")
    print(" " * 28 + " ".join(f"{r[0][:9]:>9}" for r in rows) + "     total")
    for n in names:
        print(f"{n:<28}" + " ".join(f"{r[1][n]:>9}" for r in rows) + f" {sum(r[1][n] for r in rows):>9}")


def test_counters_change_no_result(oracle_mod):
    """The census call returns the last detection's counters, and asking for it changes nothing."""
    img = dc.cases()[0].img
    k0, d0 = oracle_mod.sift_detect_and_compute(img)
    a = oracle_mod.sift_census(img)
    k1, d1 = oracle_mod.sift_detect_and_compute(img)
    assert a == oracle_mod.sift_census(img) and set(a) == set(oracle_mod.SIFT_CENSUS)
    np.testing.assert_array_equal(k0.view(np.uint8), k1.view(np.uint8))
    np.testing.assert_array_equal(d0, d1)
    assert 0 < a["accepted"] <= len(k0) + a["duplicates_removed"]  # one or more orientations per accepted candidate
    img = dc.by_size(96, 96)[0].img
    u = oracle_mod.surf_census(img, 100.0)
    k, _ = oracle_mod.surf_detect_and_compute(img, 100.0)
    assert u == oracle_mod.surf_census(img, 100.0) and set(u) == set(oracle_mod.SURF_CENSUS)
    assert u["accepted"] - u["drop_gws"] - u["drop_nang"] == len(k) > 0
    assert u["maxima"] == u["accepted"] + u["reject_all_zero"] + u["reject_abs_gt_1"]


def test_sift_cases_reach_every_branch(oracle_mod):
    rows = [(c.name, s) for c, s, _, _, _ in census(oracle_mod)]
    _table("SIFT census (oracle/sift.cpp), per case", oracle_mod.SIFT_CENSUS, rows)
    assert set(SIFT_UNREACHED) <= set(SIFT_MAY_BE_UNREACHED)
    required = [n for n in oracle_mod.SIFT_CENSUS if n not in SIFT_UNREACHED]
    total = {n: sum(s[n] for _, s in rows) for n in oracle_mod.SIFT_CENSUS}
    assert [n for n in required if total[n] <= 0] == []
    # a branch listed as unreached that an input now reaches belongs to the required ones
    assert [n for n in SIFT_UNREACHED if total[n] != 0] == []


def test_surf_cases_reach_every_branch(oracle_mod):
    rows = [(c.name, u) for c, _, u, _, _ in census(oracle_mod)]
    _table("SURF census (oracle/surf.cpp), thresholds 400 and the case's, per case", oracle_mod.SURF_CENSUS, rows)
    assert set(SURF_UNREACHED) <= set(SURF_MAY_BE_UNREACHED)
    required = [n for n in oracle_mod.SURF_CENSUS if n not in SURF_UNREACHED]
    total = {n: sum(u[n] for _, u in rows) for n in oracle_mod.SURF_CENSUS}
    assert [n for n in required if total[n] <= 0] == []
    assert [n for n in SURF_UNREACHED if total[n] != 0] == []


def test_cases_have_keypoints(oracle_mod):
    """What test_gpu_detector_regimes.py relies on: no case compares two empty lists where it is meant to
    have keypoints (4 or more; the orientation anchors exactly one, the anchor image three SURF keypoints,
    detector_cases.cases() says why), and the tiled case has its exact ties."""
    seen = set()
    for c, _, _, ks, ku in census(oracle_mod):
        print(f"{c.name:<18} {c.w:>3} x {c.h:<3} SIFT {len(ks):>4}   SURF({c.surf_thr:g}) {len(ku):>4}")
        assert len(ks) >= c.min_sift and len(ku) >= c.min_surf, c.name
        assert c.min_sift >= 1 and (c.min_surf >= 1 or (c.w, c.h) == (40, 30)), c.name
        seen.add((c.w, c.h))
    assert seen == set(dc.SIZES)
    for w, h in dc.SIZES:  # every size has SURF keypoints in some case, and SIFT ones in every case
        assert any(c.min_surf >= 4 for c in dc.by_size(w, h))
    by_name = {c.name: (s, u, ks, ku) for c, s, u, ks, ku in census(oracle_mod)}
    _, _, ks, ku = by_name["tiled"]
    assert int((np.diff(ku["response"]) == 0).sum()) >= 20  # KeypointGreater's later keys decide
    assert int((np.diff(ks["x"]) == 0).sum()) >= 20         # KeyPoint12_LessThan's later keys decide
