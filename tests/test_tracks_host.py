"""Tracks without a GPU: the ABI's struct and the numpy dtype agree, both sides name the new entry
points, carry_scale follows its rule, the numpy restatement the GPU tests compare against
(track_cases.reference) does what the header says on cases small enough to write out, the seeded
generators set what they claim to set, and on the noiseless three-view scene the reference
recovers the ratio of the two baselines."""
import os
import re

import numpy as np
import pytest

import track_cases as tc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("dvo_stream_set_tracks", "dvo_knn_stream_set_tracks", "dvo_test_tracks")
C_TYPES = {"int32_t": ("<i4", 4), "float": ("<f4", 4), "double": ("<f8", 8)}


def _header():
    return open(os.path.join(ROOT, "include", "dvo.h")).read()


def test_struct_and_dtype_agree():
    from droplet_visual_odometry_amd._native import TRACK_SCALE_DTYPE
    body = re.search(r"typedef struct \{([^}]*)\} dvo_track_scale;", _header()).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields, off = [], 0
    for decl in filter(None, (d.strip() for d in body.split(";"))):
        ctype, names = decl.split(None, 1)
        code, size = C_TYPES[ctype]
        for name in (n.strip() for n in names.split(",")):
            off = (off + size - 1) // size * size
            fields.append((name, code, off))
            off += size
    assert (off + 7) // 8 * 8 == TRACK_SCALE_DTYPE.itemsize == 32
    assert [f[0] for f in fields] == list(TRACK_SCALE_DTYPE.names)
    for name, code, o in fields:
        assert TRACK_SCALE_DTYPE.fields[name][0] == np.dtype(code), name
        assert TRACK_SCALE_DTYPE.fields[name][1] == o, name


def test_entry_points_declared_and_bound():
    from test_abi import declared_symbols
    from droplet_visual_odometry_amd import _native
    names = declared_symbols()
    for e in ENTRIES:
        assert e in names, e
        assert e in _native._SIGNATURES, e
    lib = _native.load_library()
    for e in ENTRIES:
        assert getattr(lib, e) is not None


def test_python_surface():
    from droplet_visual_odometry_amd import ops, stream
    for cls in (stream.FrameStream, stream.KnnFrameStream):
        assert callable(getattr(cls, "bind_tracks"))
    assert callable(stream.Tracks) and callable(stream.carry_scale) and callable(ops.test_tracks)


def _scales(ratio, n_common):
    from droplet_visual_odometry_amd._native import TRACK_SCALE_DTYPE
    s = np.zeros(len(ratio), TRACK_SCALE_DTYPE)
    s["ratio"], s["n_common"] = ratio, n_common
    return s


def test_carry_scale():
    from droplet_visual_odometry_amd.stream import carry_scale
    nan = np.nan
    s = _scales([0.0, 2.0, 0.5, 0.0, 3.0, 1.5, 4.0], [-1, 5, 1, 0, 7, 2, 3])
    # no anchor before pair 2: NaN until then; pair 3 has no shared point: the chain breaks there
    # and pair 4 stays NaN although it has a ratio; pair 5's own anchor starts it again
    out = carry_scale([nan, nan, 0.8, nan, nan, 0.25, nan], s)
    np.testing.assert_array_equal(out, [nan, nan, 0.8, nan, nan, 0.25, 0.25 * 4.0])
    # an anchor on pair 0 carries through every linked pair; an anchor always wins over the chain
    out = carry_scale([2.0, nan, nan, 7.0, nan, nan, nan], s)
    np.testing.assert_array_equal(out, [2.0, 2.0 * 2.0, 2.0 * 2.0 * 0.5, 7.0, 7.0 * 3.0, 7.0 * 3.0 * 1.5, 7.0 * 3.0 * 1.5 * 4.0])
    # pair 0 of a batch (n_common -1) never chains, whatever its ratio field holds
    assert np.isnan(carry_scale([nan, 1.0], _scales([9.0, 2.0], [-1, 4]))[0])
    # no threshold of its own: one shared point is enough
    np.testing.assert_array_equal(carry_scale([1.0, nan], _scales([0.0, 2.0], [-1, 1])), [1.0, 2.0])
    assert carry_scale(np.zeros(0), _scales([], [])).shape == (0,)
    with pytest.raises(ValueError):
        carry_scale([1.0], s)


def test_reference_written_out():
    """Three pairs small enough to check by hand: a duplicate trainIdx, a landmark with no
    predecessor, a match that is no landmark, and an empty pair."""
    from droplet_visual_odometry_amd._native import PAIR_RECORD_DTYPE
    recs = np.zeros(3, PAIR_RECORD_DTYPE)
    recs["R"] = np.eye(3).reshape(9)
    recs[0]["t"] = [0.0, 0.0, 1.0]
    # pair 0: matches (q, t) = (0, 7) (1, 5) (2, 7) (3, 9); all but match 1 are landmarks: ordinals 0, 1, 2
    m0 = (np.array([0, 1, 2, 3]), np.array([7, 5, 7, 9]))
    l0 = (np.array([0, 2, 3]), np.array([[0, 0, 1.0], [0, 0, 2.0], [0, 0, 3.0]]))
    # pair 1: queries 7 (twice kept in pair 0: ordinal 0 wins), 5 (pair 0's match 1 is no landmark), 9, 4
    m1 = (np.array([7, 5, 9, 4]), np.array([1, 2, 3, 0]))
    l1 = (np.array([0, 1, 2, 3]), np.array([[0, 0, 4.0], [0, 0, 1.0], [0, 0, 2.0], [0, 0, 1.0]]))
    # pair 2: no landmarks
    m2 = (np.array([1, 2]), np.array([0, 1]))
    l2 = (np.zeros(0, np.int32), np.zeros((0, 3)))
    links, sc = tc.reference([l0, l1, l2], [m0, m1, m2], recs)
    assert [list(x) for x in links] == [[-1, -1, -1], [0, -1, 2, -1], []]
    assert list(sc["n_common"]) == [-1, 2, 0] and list(sc["n_prev"]) == [0, 3, 4]
    # ratios |Xa + (0, 0, 1)| / |Xb|: (1 + 1) / 4 and (3 + 1) / 2; lower median and q1 the first, q3 the first too
    assert (sc[1]["ratio"], sc[1]["q1"], sc[1]["q3"]) == (0.5, 0.5, 0.5)
    assert (sc[0]["ratio"], sc[2]["ratio"], sc[2]["q3"]) == (0.0, 0.0, 0.0)


def test_order_statistics_ranks():
    for n in (1, 2, 3, 4, 5, 8, 9):
        v = np.arange(1, n + 1, dtype=np.float64)
        _, sc = tc.reference(*tc.exact_ratios(v[::-1]))
        assert sc[1]["n_common"] == n
        assert (sc[1]["ratio"], sc[1]["q1"], sc[1]["q3"]) == (v[(n - 1) // 2], v[(n - 1) // 4], v[3 * (n - 1) // 4]), n


def test_ratio_arithmetic_order():
    """The stated order is not the only one: a fused or re-associated sum differs in the last bit
    for some inputs, and the reference keeps the header's."""
    r = np.random.RandomState(3)
    a, b = r.uniform(-5, 5, (4000, 3)), r.uniform(0.5, 40, (4000, 3))
    R, t = tc._rotation(r), r.normal(size=3)
    got = tc.ratios_of(a, b, R, t)
    y = a @ R.T + t
    other = np.linalg.norm(y, axis=1) / np.linalg.norm(b, axis=1)
    assert np.allclose(got, other, rtol=1e-14) and (got != other).any()
    i = 17
    yy = [((R[k, 0] * a[i, 0] + R[k, 1] * a[i, 1]) + R[k, 2] * a[i, 2]) + t[k] for k in range(3)]
    want = np.sqrt((yy[0] * yy[0] + yy[1] * yy[1]) + yy[2] * yy[2]) / np.sqrt((b[i, 0] * b[i, 0] + b[i, 1] * b[i, 1]) + b[i, 2] * b[i, 2])
    assert got[i] == want


def test_chain_sets_its_sizes():
    spec = [(300, 200, 0), (300, 260, 63), (280, 0, 0), (300, 262, 0), (300, 256, 255)]
    lms, matches, recs = tc.chain(spec, kp_cap=900, seed=5, dups=3)
    links, sc = tc.reference(lms, matches, recs)
    assert list(sc["n_common"]) == [-1, 63, 0, 0, 255]
    assert list(sc["n_prev"]) == [0, 200, 260, 0, 262]
    for p, (m, count, _) in enumerate(spec):
        assert len(lms[p][0]) == count and len(matches[p][0]) == m
        if count:  # the duplicates are there
            assert count - 3 <= len(np.unique(matches[p][1][lms[p][0]])) <= count - 1
    assert np.isfinite(sc["ratio"]).all() and (sc["ratio"][[1, 4]] > 0).all()


def test_scene_recovers_the_baseline_ratio(oracle_mod):
    """Noiseless pixels: the median ratio is |t_b| / |t_a| to within 4x the largest deviation
    measured over the kept sizes (track_cases.NOISELESS_DEV; the dropped sizes are in DROPPED)."""
    true = tc.T_B / tc.T_A
    for m in tc.SCENE_SIZES:
        links, sc = tc.scene_reference(oracle_mod, m)
        dev = sc[1]["ratio"] / true - 1
        print("m", m, "n_common", sc[1]["n_common"], "n_prev", sc[1]["n_prev"], "ratio", sc[1]["ratio"], "dev %.3e" % dev,
              "q1 %.5f q3 %.5f" % (sc[1]["q1"], sc[1]["q3"]))
        assert sc[1]["n_common"] >= m // 2 and sc[0]["n_common"] == -1
        assert abs(dev) <= tc.SCENE_BOUND, (m, dev)
        # matches are point for point, so a link is the ordinal of the same match in pair 0
        assert (links[1] >= -1).all() and (links[0] == -1).all()
