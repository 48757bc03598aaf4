"""Every RANSAC hypothesis the production kernels evaluate, against the oracle's per-hypothesis
loop (oracle.ransac_hypotheses), not only the hypothesis that wins.

ops.test_ransac_hypotheses runs the production launches under three schedules and returns what
they left in the GeomArgs arrays:
  CALL          dvo_find_essential_mat's launch: ransac_dk_wide_kernel, ransac_stage_c_row_kernel,
                ransac_score_kernel<kScoreHypsCall>
  BATCH_ONE     the batch kernels over all hypotheses as one round: ransac_dk_kernel in its passes
                (parking and compaction), ransac_stage_c_kernel, ransac_score_kernel<kScoreHyps>
  BATCH_ROUNDS  the stream's rounds (kRansacBounds), each starting from the last one's state
For every evaluated hypothesis the subset, the model count and the models are the oracle's bit for
bit (NaNs compare as NaNs: a generated NaN's sign differs between the oracle's host and the device,
and most models of "identical" are NaN), and so is the solver branch (path) where the schedule
keeps it.

Counts: the score kernel stops counting a model that cannot exceed bail = max(best count at the
start of its round, 4) and stores the partial count.  So with B_h = max(4, the largest oracle count
of any model of a hypothesis before h's round), cnt == oracle where the oracle's count is above
B_h, and cnt <= oracle elsewhere.  In the one-round schedules B_h is 4, and the share of models
checked only by <= (oracle count <= 4) is capped at 1 %.  Measured with the oracle's own counts
(test_oracle_kats.py::test_ransac_hypothesis_sets_reach_their_regimes prints them):
  repeated 0 / 2,812   collinear 0 / 2,268   integer 0 / 2,780   pure_rotation 0 / 3,610
  realistic50 0 / 2,632   sparse25 0 / 2,658   over_chunk 0 / 2,664   undecided_tail 0 / 2,022
"identical" is exempt (596 of its 620 models have <= 4 inliers); it is here for its 596 of 600
hypotheses on the trimmed-degree solver (path 1).

"undecided_tail" (a tiny focal length: every point test is left to f64; three inlier points past
the first score chunk) is there for the early exit itself: a model whose first chunk went to the
deferred list has counted nothing when the 3-point last chunk starts, and only the exit's
deferred-test term keeps it being scored.  Without that term its counts come out up to 3 short.

Not reached: path 2, the coincident-root redo (solve_poly10 inside stage C).  No hypothesis of
these sets takes it in the oracle, and a CPU search over 240,000 hypotheses of mirrored, integer,
grid and repeated-point configurations found none, so nothing here asserts it.
"""
import numpy as np
import pytest

import ransac_cases
from ransac_cases import N_HYP

pytestmark = pytest.mark.gpu

SCHEDULES = ("CALL", "BATCH_ONE", "BATCH_ROUNDS")
PROB = 0.999
_RUNS = {}


def _run(gpu_ctx, schedule, names):
    """One launch of the named sets (cached: the multi-pair test compares with the single runs)."""
    from droplet_visual_odometry_amd import ops
    key = (schedule,) + tuple(names)
    if key not in _RUNS:
        sets = _multi_sets() if len(names) > 1 else ransac_cases.hypothesis_sets()
        _RUNS[key] = ops.test_ransac_hypotheses([sets[n][:2] for n in names], sets[names[0]][2], N_HYP, schedule,
                                                prob=PROB, ctx=gpu_ctx)
    return _RUNS[key]


def _bits(a):
    """The doubles' bit patterns, every NaN as one pattern: a NaN an operation generates has the
    sign bit set on the oracle's x86 host and clear on the device ("identical" has NaN models)."""
    a = np.ascontiguousarray(a, np.float64)
    u = a.view(np.uint64).copy()
    u[np.isnan(a)] = 0x7FF8000000000000
    return u


def _pair(res, p):
    return {k: (v if k in ("bounds", "parked") or v is None else v[p]) for k, v in res.items()}


def _bail_bound(ref, bounds):
    """B_h per hypothesis: max(4, the largest oracle count before the start of h's round)."""
    valid = np.arange(10)[None, :] < ref["nmod"][:, None]
    best = np.where(valid, ref["cnt"], 0).max(axis=1)          # per hypothesis
    before = np.concatenate([[0], np.maximum.accumulate(best)])  # before[h]: max over hypotheses < h
    h = np.arange(N_HYP)
    rnd = np.searchsorted(np.asarray(bounds, np.int64), h, side="right")  # h < bounds[rnd]
    start = np.where(rnd == 0, 0, np.asarray(bounds, np.int64)[np.maximum(rnd, 1) - 1])
    return np.maximum(4, before[np.minimum(start, N_HYP)])


def _check_pair(oracle_mod, got, name, schedule, sets=None):
    p1, p2, K = (sets or ransac_cases.hypothesis_sets())[name]
    m = len(p1)
    ref = ransac_cases.oracle_hypotheses(oracle_mod, name)
    one = schedule != "BATCH_ROUNDS"
    done = got["nmod"] != -1
    n_done = int(done.sum())
    assert done[:n_done].all(), "the evaluated hypotheses are not a prefix"
    if one:
        assert n_done == N_HYP
        np.testing.assert_array_equal(got["bounds"], [1 << 30])
    else:
        _, _, iters = oracle_mod.find_essential(p1, p2, K, prob=PROB, max_iters=N_HYP)
        assert n_done >= iters, (n_done, iters)
        assert len(got["bounds"]) >= 2 and got["bounds"][-1] == 1 << 30 and (np.diff(got["bounds"]) > 0).all()
    s = slice(0, n_done)
    np.testing.assert_array_equal(got["subsets"][s], ref["subsets"][s])
    np.testing.assert_array_equal(got["nmod"][s], ref["nmod"][s])
    valid = np.zeros((N_HYP, 10), bool)
    valid[s] = np.arange(10)[None, :] < ref["nmod"][s, None]
    np.testing.assert_array_equal(_bits(got["models"][valid]), _bits(ref["models"][valid]))
    assert not got["models"][~valid].view(np.uint64).any(), "a model outside [0, nmod) was written"
    if got["path"] is not None:
        np.testing.assert_array_equal(got["path"][s], ref["path"][s])
    # counts: exact above the bail bound, never more below it
    B = np.broadcast_to(_bail_bound(ref, got["bounds"])[:, None], (N_HYP, 10))
    exact = valid & (ref["cnt"] > B)
    weak = valid & ~exact
    np.testing.assert_array_equal(got["cnt"][exact], ref["cnt"][exact])
    assert (got["cnt"][weak] <= ref["cnt"][weak]).all() and (got["cnt"][weak] >= 0).all()
    assert not got["cnt"][~valid].any(), "a count outside [0, nmod) was written"
    if one and name in ransac_cases.CAPPED_SETS:
        assert weak.sum() <= 0.01 * valid.sum(), (name, int(weak.sum()), int(valid.sum()))
    want = oracle_mod.ransac_replay(ref["nmod"], ref["cnt"], m, PROB, N_HYP)
    assert tuple(int(v) for v in got["state"]) == want, (got["state"], want)
    return n_done


@pytest.mark.parametrize("name", ransac_cases.HYPOTHESIS_SETS)
@pytest.mark.parametrize("schedule", SCHEDULES)
def test_every_hypothesis_equals_the_oracle(gpu_ctx, oracle_mod, schedule, name):
    got = _pair(_run(gpu_ctx, schedule, (name,)), 0)
    n_done = _check_pair(oracle_mod, got, name, schedule)
    print(f"{schedule} {name}: {n_done} hypotheses evaluated, state {got['state'].tolist()}, parked {got['parked']}")


@pytest.mark.parametrize("schedule", ("CALL", "BATCH_ONE"))
def test_trimmed_degree_solver_is_reached(gpu_ctx, schedule):
    path = _run(gpu_ctx, schedule, ("identical",))["path"][0]
    assert (path == 1).sum() > 300 and (path == 0).any(), np.bincount(path + 1).tolist()


def test_batch_round_parks_polynomials_in_both_passes(gpu_ctx):
    """realistic50 as one batch round: polynomials are parked after Durand-Kerner pass 0 and again
    after pass 1, so the roots compared above went through parking, compaction and resumption."""
    parked = _run(gpu_ctx, "BATCH_ONE", ("realistic50",))["parked"]
    print("parked after pass 0, 1, 2, 3:", parked.tolist(), "of", N_HYP)
    assert parked[0] > 0 and parked[1] > 0
    assert parked[0] <= N_HYP and parked[1] <= parked[0]


def test_all_rounds_run_on_sparse25(gpu_ctx):
    """niters stays at the cap, so the last round of the batch schedule reaches hypothesis 599."""
    got = _pair(_run(gpu_ctx, "BATCH_ROUNDS", ("sparse25",)), 0)
    assert (got["nmod"] != -1).all() and got["state"][0] == N_HYP


MULTI = ("realistic50", "empty", "five", "integer", "sparse25")


def _multi_sets():
    sets = dict(ransac_cases.hypothesis_sets())
    p1, p2, K = sets["integer"]
    sets["empty"] = (p1[:0], p2[:0], K)
    sets["five"] = (p1[:5].copy(), p2[:5].copy(), K)  # m == modelPoints: one direct solve, no RANSAC
    return sets


@pytest.mark.parametrize("schedule", ("BATCH_ONE", "BATCH_ROUNDS"))
def test_pairs_of_one_launch_equal_single_launches(gpu_ctx, oracle_mod, schedule):
    """Five pairs in one launch, an empty one and a five-point one between full ones (the work-list
    pair lookup over a run of pairs without hypotheses, the packed record layout): every pair's
    outputs are those of the pair launched alone, and the oracle's."""
    sets = _multi_sets()
    multi = _run(gpu_ctx, schedule, MULTI)
    for p, name in enumerate(MULTI):
        got = _pair(multi, p)
        if name in ("empty", "five"):
            from droplet_visual_odometry_amd import ops
            alone = _pair(ops.test_ransac_hypotheses([sets[name][:2]], ransac_cases.K_VGA, N_HYP, schedule, prob=PROB,
                                                     ctx=gpu_ctx), 0)
        else:
            alone = _pair(_run(gpu_ctx, schedule, (name,)), 0)
            _check_pair(oracle_mod, got, name, schedule, sets)
        for k in ("subsets", "nmod", "models", "cnt", "state", "path"):
            if got[k] is not None:
                np.testing.assert_array_equal(got[k], alone[k], err_msg=f"pair {p} ({name}) {k}")
    empty, five = _pair(multi, 1), _pair(multi, 2)
    assert (empty["nmod"] == -1).all() and empty["state"].tolist() == [0, N_HYP, 0, -1, -1]
    E5, _, _ = oracle_mod.find_essential(*sets["five"][:2], sets["five"][2], prob=PROB, max_iters=N_HYP)
    k = 0 if E5 is None else len(E5) // 3
    assert five["nmod"][0] == k and (five["nmod"][1:] == -1).all()
    assert five["state"].tolist() == [0, N_HYP, 0, -1, -1]
    if k:
        np.testing.assert_array_equal(_bits(five["models"][0, :k].reshape(-1)), _bits(E5.reshape(-1)))
