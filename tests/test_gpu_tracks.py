"""Tracks on the device (dvo_stream_set_tracks, stream.Tracks): the landmarks of consecutive pairs
joined on the keypoint they share, and per pair the order statistics of the baseline ratios.
Every comparison is exact: links equal, and ratio, q1, q3 bit-identical to the numpy restatement
of the header's contract (track_cases.reference); every byte outside the written link slots
keeps the 0xA5 the buffers were filled with."""
import numpy as np
import pytest

import track_cases as tc
from conftest import synth_frames

pytestmark = pytest.mark.gpu

FILL = 0xA5
FILL32 = np.frombuffer(bytes([FILL] * 4), np.int32)[0]
ORB_SIZES = [(320, 240, 300), (640, 480, 500)]
SMALL = ORB_SIZES[0]
BLANK = 3


def _same_scales(got, want):
    assert list(got["n_common"]) == list(want["n_common"])
    assert list(got["n_prev"]) == list(want["n_prev"])
    for f in ("ratio", "q1", "q3"):  # bit for bit
        assert got[f].tobytes() == want[f].tobytes(), (f, got[f], want[f])


def _hook(gpu_ctx, lms, matches, recs, kp_cap, stride, cap_out=None):
    """The hook on a case; checks it against the reference at the full cap or at cap_out."""
    from droplet_visual_odometry_amd import ops
    want_links, want = tc.reference(lms, matches, recs)
    cap = max(max(len(a[0]) for a in lms), 1)
    lm, count, mq, mt, m = tc.pack(lms, matches, recs, cap, stride)
    co = cap if cap_out is None else cap_out
    link = np.full((len(lms), co), FILL32, np.int32)
    link, scale = ops.test_tracks(lm, count, mq, mt, m, recs, kp_cap, cap_out=co, link=link, ctx=gpu_ctx)
    _same_scales(scale, want)
    for p, w in enumerate(want_links):
        n = min(len(w), co)
        np.testing.assert_array_equal(link[p, :n], w[:n], err_msg=str(p))
        assert (link[p, n:] == FILL32).all(), p
    return want_links, want


# ---- 1. the hook at sizes around the tiles of 256 landmarks ------------------------------------
# (matches, landmarks, n_common): n_common 0 1 2 3 4 63 64 65 255 256 257 513, landmark counts
# around 256 and 512, a pair without landmarks, its successor, and a five-match pair
SPEC = [(600, 520, 0), (600, 300, 0), (600, 255, 1), (600, 256, 2), (600, 257, 3), (600, 511, 4), (600, 512, 63),
        (600, 513, 64), (650, 600, 65), (700, 640, 255), (700, 600, 256), (700, 650, 257), (700, 690, 513),
        (700, 0, 0), (700, 400, 0), (5, 5, 3)]
STRIDE, KP_CAP = 700, 2200
_CHAIN = {}


def _chain():
    if not _CHAIN:
        _CHAIN["case"] = tc.chain(SPEC, KP_CAP, seed=11, dups=3)
    return _CHAIN["case"]


def test_hook_sizes(gpu_ctx):
    lms, matches, recs = _chain()
    links, want = _hook(gpu_ctx, lms, matches, recs, KP_CAP, STRIDE)
    print("n_common", list(want["n_common"]), "n_prev", list(want["n_prev"]))
    assert list(want["n_common"]) == [-1] + [s[2] for s in SPEC[1:]]
    assert want["n_prev"][14] == 0 and want["n_common"][14] == 0 and len(links[14]) == 400  # the predecessor is empty
    assert (links[0] == -1).all() and want["n_common"][0] == -1
    # duplicates in the predecessor: some landmark links to a train index two landmarks hold, and takes the first
    hit = 0
    for p in range(1, len(SPEC)):
        t_prev = matches[p - 1][1][lms[p - 1][0]]
        for o in np.flatnonzero(links[p] >= 0):
            same = np.flatnonzero(t_prev == matches[p][0][lms[p][0][o]])
            assert links[p][o] == same[0]
            hit += len(same) > 1
    assert hit > 0


def test_hook_cap_out(gpu_ctx):
    """A caller's cap below the counts: the same scales, the first 16 links, and links >= 16."""
    lms, matches, recs = _chain()
    links, _ = _hook(gpu_ctx, lms, matches, recs, KP_CAP, STRIDE, cap_out=16)
    assert max(int(l[:16].max()) for l in links if len(l)) >= 16


def test_hook_beyond_lds(gpu_ctx):
    """More shared landmarks than the select kernel keeps in LDS (2048): at the limit and past it."""
    spec = [(2400, 2300, 0), (2400, 2200, 2048), (2400, 2350, 2049), (2400, 2390, 2300)]
    lms, matches, recs = tc.chain(spec, 7300, seed=12, dups=2)
    _, want = _hook(gpu_ctx, lms, matches, recs, 7300, 2400)
    assert list(want["n_common"]) == [-1, 2048, 2049, 2300]


# ---- 2. the radix select: ratio sets that decide in every pass ---------------------------------
def _bits(base, add):
    return (np.float64(base).view(np.uint64) + np.asarray(add, np.uint64)).view(np.float64)


def _select_sets():
    r = np.random.RandomState(21)
    one = np.array([1.0]).view(np.uint64)[0]
    sets = {
        "all_equal": np.full(300, 1.37),
        "one": np.array([0.75]),
        "two": np.array([3.0, 0.5]),
        "lowest_byte": _bits(1.25, r.randint(0, 256, 200)),
        "exponent_only": 2.0 ** r.permutation(np.arange(-400, 400, 3)),
        "quartile_ties": r.permutation(np.repeat([1.0, 2.0, 3.0, 5.0], [30, 41, 2, 28])),
        "every_byte": r.uniform(1, 2, 777),
        "wide": 10.0 ** r.uniform(-140, 140, 513),
    }
    for b in range(1, 7):  # sets that agree above byte b and are decided in that pass alone
        sets[f"byte_{b}"] = (one + (r.randint(0, 256, 130).astype(np.uint64) << np.uint64(8 * b))).view(np.float64)
    return sets


@pytest.mark.parametrize("name", sorted(_select_sets()))
def test_hook_select(gpu_ctx, name):
    v = _select_sets()[name]
    lms, matches, recs = tc.exact_ratios(v)
    _, want = _hook(gpu_ctx, lms, matches, recs, len(v), len(v))
    s = np.sort(v)
    n = len(v)
    assert want[1]["n_common"] == n  # and the construction gives exactly these ratios
    assert (want[1]["ratio"], want[1]["q1"], want[1]["q3"]) == (s[(n - 1) // 2], s[(n - 1) // 4], s[3 * (n - 1) // 4])


def test_hook_select_magnitudes(gpu_ctx):
    """Ratios from 1e-300 to 1e300 by scaling XYZ (squares stay in range; t is made tiny, or
    |R Xa + t| would never fall below |t| = 1)."""
    lms, matches, recs = tc.chain([(500, 400, 0), (500, 450, 300), (500, 470, 333)], 1600, seed=13, decades=149.0,
                                  t_len=1e-152)
    links, want = _hook(gpu_ctx, lms, matches, recs, 1600, 500)
    on = np.flatnonzero(links[1] >= 0)
    r = tc.ratios_of(lms[0][1][links[1][on]], lms[1][1][on], recs[0]["R"], recs[0]["t"])
    assert np.isfinite(r).all() and r.min() < 1e-200 and r.max() > 1e200


# ---- 3.-6. the ORB stream ----------------------------------------------------------------------
def _filled(n_pairs, cap, device="cuda"):
    import torch
    from droplet_visual_odometry_amd.stream import Landmarks, Tracks
    lm, tr = Landmarks(n_pairs, cap, device), Tracks(n_pairs, cap, device)
    for t in (lm.entries, lm.counts, tr.links, tr.scales):
        t.view(torch.uint8).fill_(FILL)
    return lm, tr


def _stream_reference(fs, lm, recs, n_pairs):
    """The reference from the stream's own landmarks (a Landmarks that holds every one), matches and records."""
    lms, matches = [], []
    none = np.zeros(0, np.int32)
    for i in range(n_pairs):
        assert lm.count(i) <= lm.cap
        e = lm.numpy(i)
        lms.append((e["match"], np.stack([e["X"], e["Y"], e["Z"]], 1) if len(e) else np.zeros((0, 3))))
        m = fs.matches(i) if len(e) else None
        matches.append((m["queryIdx"], m["trainIdx"]) if len(e) else (none, none))
    return tc.reference(lms, matches, recs)


def _check_stream(lm, tr, want_links, want):
    raw = tr.links.cpu().numpy()
    _same_scales(tr.scales_numpy(), want)
    for p, w in enumerate(want_links):
        np.testing.assert_array_equal(tr.numpy(p, lm.count(p)), w, err_msg=str(p))
        assert (raw[p, len(w):] == FILL32).all(), p


_ORB = {}


def _orb(gpu_ctx, size):
    if size not in _ORB:
        import torch
        from droplet_visual_odometry_amd.stream import FrameStream
        W, H, NF = size
        frames, K = synth_frames(W, H, range(6))
        cap = NF + 37
        fs = FrameStream(W, H, K, nfeatures=NF, max_frames=6, ctx=gpu_ctx)
        lm, tr = _filled(5, cap)
        fs.bind_landmarks(lm)
        fs.bind_tracks(tr)
        rec = fs.process(torch.from_numpy(frames).cuda())
        fs.sync()
        recs = FrameStream.records_numpy(rec, 5)
        _ORB[size] = dict(frames=frames, K=K, cap=cap, recs=recs, lm=lm, tr=tr, fs=fs,
                          want=_stream_reference(fs, lm, recs, 5))
    return _ORB[size]


@pytest.mark.parametrize("size", ORB_SIZES)
def test_orb_stream_process(gpu_ctx, size):
    r = _orb(gpu_ctx, size)
    links, want = r["want"]
    print(size, "landmarks", [r["lm"].count(i) for i in range(5)], "n_common", list(want["n_common"]),
          "ratio", list(want["ratio"]), "q1", list(want["q1"]), "q3", list(want["q3"]))
    assert want["n_common"][0] == -1 and (want["n_common"][1:] >= 3).all()
    _check_stream(r["lm"], r["tr"], links, want)


def test_orb_failed_pairs(gpu_ctx):
    import torch
    from droplet_visual_odometry_amd.stream import FrameStream
    r = _orb(gpu_ctx, SMALL)
    frames = r["frames"].copy()
    frames[BLANK] = 90
    fs = r["fs"]
    lm, tr = _filled(5, r["cap"])
    fs.bind_landmarks(lm)
    fs.bind_tracks(tr)
    rec = fs.process(torch.from_numpy(frames).cuda())
    fs.sync()
    recs = FrameStream.records_numpy(rec, 5)
    links, want = _stream_reference(fs, lm, recs, 5)
    sc = tr.scales_numpy()
    print("status", list(recs["status"]), "n_common", list(sc["n_common"]), "n_prev", list(sc["n_prev"]))
    for i in (BLANK - 1, BLANK):  # the pairs that touch the blank frame
        assert recs[i]["status"] != 0 and lm.count(i) == 0 and sc[i]["n_common"] == 0, i
    assert sc[BLANK - 1]["n_prev"] == lm.count(BLANK - 2) > 0
    # the pair after them has landmarks but a failed predecessor
    assert lm.count(BLANK + 1) > 0 and sc[BLANK + 1]["n_common"] == 0 and sc[BLANK + 1]["n_prev"] == 0
    assert (tr.numpy(BLANK + 1, lm.count(BLANK + 1)) == -1).all()
    assert sc[1]["n_common"] >= 3
    _check_stream(lm, tr, links, want)


def test_orb_submit_equals_process(gpu_ctx):
    """Three batches submitted back to back, tracks on the first two, equal the same batches
    processed one at a time.  A later batch's matching has overwritten the stream's match indices
    when an earlier one retires: this is the test of the per-set index copy."""
    import torch
    from droplet_visual_odometry_amd.stream import FrameStream
    W, H, NF = SMALL
    sizes, cap = [4, 3, 4], NF + 37
    starts = np.concatenate([[0], np.cumsum(np.array(sizes) - 1)])[:-1]
    frames, K = synth_frames(W, H, range(int(starts[-1] + sizes[-1])))
    dev = torch.from_numpy(frames).cuda()
    a = FrameStream(W, H, K, nfeatures=NF, max_frames=max(sizes), ctx=gpu_ctx)
    b = FrameStream(W, H, K, nfeatures=NF, max_frames=max(sizes), ctx=gpu_ctx)
    want = []
    for k, (s0, m) in enumerate(zip(starts, sizes)):
        lm, tr = _filled(m - 1, cap)
        a.bind_landmarks(lm)
        if k < 2:
            a.bind_tracks(tr)
        rec = a.process(dev[s0:s0 + m])
        a.sync()
        recs = FrameStream.records_numpy(rec, m - 1)
        if k < 2:  # and the process side is right to begin with
            _check_stream(lm, tr, *_stream_reference(a, lm, recs, m - 1))
        want.append((recs, lm, tr))
    assert sum(int((w[2].scales_numpy()["n_common"] > 0).sum()) for w in want[:2]) >= 2
    bufs = [_filled(m - 1, cap) for m in sizes]
    recs = [b.new_records(m - 1) for m in sizes]
    torch.cuda.synchronize()
    for k, (s0, m, (lm, tr), rec) in enumerate(zip(starts, sizes, bufs, recs)):
        b.bind_landmarks(lm)
        if k < 2:
            b.bind_tracks(tr)
        b.submit(dev[s0:s0 + m], rec, wait_torch=False)
    b.drain()
    b.sync()
    for k, m in enumerate(sizes):
        lm, tr = bufs[k]
        assert FrameStream.records_numpy(recs[k], m - 1).tobytes() == want[k][0].tobytes(), k
        for got, ref in ((lm.entries, want[k][1].entries), (lm.counts, want[k][1].counts), (tr.links, want[k][2].links),
                         (tr.scales, want[k][2].scales)):
            assert got.cpu().numpy().tobytes() == ref.cpu().numpy().tobytes(), k
    assert (bufs[2][1].links.cpu().numpy() == FILL32).all()  # the third batch bound no tracks
    a.close()
    b.close()


def test_orb_one_shot_and_default(gpu_ctx):
    import torch
    from droplet_visual_odometry_amd._native import DVO_EINVAL
    from droplet_visual_odometry_amd.stream import FrameStream, Tracks
    r = _orb(gpu_ctx, SMALL)
    W, H, NF = SMALL
    dev = torch.from_numpy(r["frames"]).cuda()
    fs, cap = r["fs"], r["cap"]
    lib = fs.ctx.lib

    def untouched(tr):
        return (tr.links.cpu().numpy() == FILL32).all() and (tr.scales.cpu().numpy() == FILL).all()

    # a stream that never binds tracks: a landmarks-only batch writes these bytes
    plain = FrameStream(W, H, r["K"], nfeatures=NF, max_frames=6, ctx=gpu_ctx)
    lm0, _ = _filled(5, cap)
    plain.bind_landmarks(lm0)
    plain.process(dev)
    plain.sync()
    # one-shot: a bound batch, then a landmarks-only batch that leaves the refilled Tracks alone
    # and writes the landmark bytes of the stream that never bound tracks
    lm, tr = _filled(5, cap)
    fs.bind_landmarks(lm)
    fs.bind_tracks(tr)
    fs.process(dev)
    fs.sync()
    _check_stream(lm, tr, *r["want"])
    lm, tr = _filled(5, cap)
    fs.bind_landmarks(lm)
    rec = fs.process(dev)
    fs.sync()
    assert untouched(tr)
    assert lm.entries.cpu().numpy().tobytes() == lm0.entries.cpu().numpy().tobytes()
    assert lm.counts.cpu().numpy().tobytes() == lm0.counts.cpu().numpy().tobytes()
    assert FrameStream.records_numpy(rec, 5).tobytes() == r["recs"].tobytes()
    # a cleared tracks binding writes nothing, the landmarks still arrive
    lm, tr = _filled(5, cap)
    fs.bind_landmarks(lm)
    fs.bind_tracks(tr)
    fs.bind_tracks(None)
    fs.process(dev)
    fs.sync()
    assert untouched(tr) and lm.count(0) > 0
    # links only and scales only
    lm, tr = _filled(5, cap)
    fs.bind_landmarks(lm)
    assert lib.dvo_stream_set_tracks(fs.h, tr.links.data_ptr(), None) == 0
    fs.process(dev)
    fs.sync()
    assert (tr.scales.cpu().numpy() == FILL).all()
    for p, w in enumerate(r["want"][0]):
        np.testing.assert_array_equal(tr.numpy(p, lm.count(p)), w)
    lm, tr = _filled(5, cap)
    fs.bind_landmarks(lm)
    assert lib.dvo_stream_set_tracks(fs.h, None, tr.scales.data_ptr()) == 0
    fs.process(dev)
    fs.sync()
    assert (tr.links.cpu().numpy() == FILL32).all()
    _same_scales(tr.scales_numpy(), r["want"][1])
    # tracks go with a pending landmark binding
    with pytest.raises(ValueError):
        fs.bind_tracks(tr)
    assert lib.dvo_stream_set_tracks(fs.h, tr.links.data_ptr(), tr.scales.data_ptr()) == DVO_EINVAL
    fs.bind_landmarks(lm)
    with pytest.raises(ValueError):  # another cap than the Landmarks'
        fs.bind_tracks(Tracks(5, cap + 1, "cuda"))
    # pairs that share no frame: Python refuses before the call ...
    lm, tr = _filled(5, cap)
    fs.bind_landmarks(lm)
    fs.bind_tracks(tr)
    with pytest.raises(ValueError):
        fs.process_pairs(dev)
    # ... and the library refuses the call and consumes both bindings: the next batch writes nothing
    rec = fs.new_records(3)
    torch.cuda.synchronize()
    assert lib.dvo_stream_process_pairs(fs.h, dev.data_ptr(), 3, dev.stride(0), dev.stride(1), rec.data_ptr()) == DVO_EINVAL
    fs._lm_next = fs._tr_next = None  # what the wrapper holds for the call it did not make
    fs.process(dev)
    fs.sync()
    assert untouched(tr) and (lm.entries.cpu().numpy() == FILL).all()
    plain.close()


# ---- 7. the k-NN stream ------------------------------------------------------------------------
@pytest.mark.parametrize("detector", ("sift", "surf"))
def test_knn_stream(gpu_ctx, detector):
    import torch
    from droplet_visual_odometry_amd._native import DVO_EINVAL
    from droplet_visual_odometry_amd.stream import KnnFrameStream
    W, H, n, cap = 640, 480, 4, 4096
    frames, K = synth_frames(W, H, range(n))
    dev = torch.from_numpy(frames).cuda()
    st = KnnFrameStream(W, H, K, n, detector=detector, feat_cap=4096, ctx=gpu_ctx)
    lm, tr = _filled(n - 1, cap)
    st.bind_landmarks(lm)
    st.bind_tracks(tr)
    rec = st.process(dev)
    st.sync()
    recs = st.records_numpy(rec, n - 1)
    assert (recs["status"] == 0).all()
    links, want = _stream_reference(st, lm, recs, n - 1)
    dup = 0
    for i in range(n - 1):
        t = st.matches(i)["trainIdx"][lm.numpy(i)["match"]]
        dup += len(t) - len(np.unique(t))
    print(detector, "landmarks", [lm.count(i) for i in range(n - 1)], "n_common", list(want["n_common"]),
          "ratio", list(want["ratio"]), "duplicate trainIdx among landmarks", dup)
    assert (want["n_common"][1:] > 0).all()
    _check_stream(lm, tr, links, want)
    # the two-phase call: detect() leaves both bindings for finish()
    lm2, tr2 = _filled(n - 1, cap)
    st.bind_landmarks(lm2)
    st.bind_tracks(tr2)
    st.detect(dev)
    st.finish()
    st.sync()
    assert tr2.links.cpu().numpy().tobytes() == tr.links.cpu().numpy().tobytes()
    assert tr2.scales.cpu().numpy().tobytes() == tr.scales.cpu().numpy().tobytes()
    # one-shot here too, and tracks go with a pending landmark binding
    tr2.links.view(torch.uint8).fill_(FILL)
    st.process(dev)
    st.sync()
    assert (tr2.links.cpu().numpy() == FILL32).all()
    with pytest.raises(ValueError):
        st.bind_tracks(tr2)
    assert st.ctx.lib.dvo_knn_stream_set_tracks(st.h, tr2.links.data_ptr(), tr2.scales.data_ptr()) == DVO_EINVAL
    st.close()
