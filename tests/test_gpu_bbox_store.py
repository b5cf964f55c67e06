"""GPU: the appearance store of include/obvi_bbox_store.h against the model of tests/bbox_store_cases.py, the restatement of tests/bbox_frontend_cases.py and the
stateless entry.  A round over stored views must give the restatement's integers exactly, the stateless entry's scores byte for byte (the same views flattened in
(frame, camera) order: both entries run the same device code) and the restatement's scores within (V + 2) 2^-53 relative (cases.score_bound, derived, not
measured).  A commit must store what the host path stores: the ids of the frame features inside the box in the caller's feature order.  The store's stats must be
the model's after every call: growth and compaction follow the rule the header documents.  The sizes are the edges the stateless test names."""
import ctypes as C

import numpy as np
import pytest

import bbox_frontend_cases as cases
import bbox_store_cases as store_cases
import helpers
import obvi_ba

pytestmark = pytest.mark.gpu
INVALID, NUMERICAL = -1, -6


@pytest.fixture(scope="module")
def ba():
    h = helpers.product_ba()
    yield h
    h.close()


@pytest.fixture
def make_store(ba):
    made = []

    def make(handle=None, **options):
        made.append(obvi_ba.BboxStore(handle or ba, **options))
        return made[-1]
    yield make
    for s in made:
        s.close()


def lds_limit():
    lib = C.CDLL(helpers.PRODUCT_LIB)
    lib.obvi_bbox_frontend_lds_feature_limit.restype = C.c_int64
    return int(lib.obvi_bbox_frontend_lds_feature_limit())


def params_of(case):
    return obvi_ba.BboxFrontendParams(case["inflation"], case["min_overlap"])


def same_state(store, model, what=""):
    """views of every owner and the stats, against the model."""
    st = store.stats()
    assert {k: getattr(st, k) for k in store_cases.STATS} == model.stats(), what
    for o in model.owners:
        assert store.views(o) == model.views(o), (what, o)
        assert store.view_sizes(o) == (len(model.owners[o]), sum(len(ids) for ids in model.owners[o].values())), (what, o)


def check_round(ba, store, model, frame, cand_owner, cand_label, r=None):
    """One round over stored views against the restatement and the stateless entry; returns (case, restated round, outputs)."""
    case = store_cases.round_case(model, frame, cand_owner, cand_label)
    r = r or cases.restate(case)
    in_box, count, overlap, match, score = store.associate(case["feat_id"], case["feat_pixel"], case["box_corners"], case["box_label"], cand_owner, case["cand_label"], params_of(case))
    assert np.array_equal(in_box, r.in_box) and np.array_equal(count, r.count) and np.array_equal(overlap, r.overlap) and np.array_equal(match, r.is_match)
    stateless = ba.bbox_associate(*cases.arrays(case), params=params_of(case))
    for got, want in zip((in_box, count, overlap, match, score), stateless):
        assert got.tobytes() == want.tobytes()                                       # the scores byte for byte, NaN where nothing was written
    worst = 0.0
    for b, c in zip(*np.nonzero(r.is_match)):
        want, bound = float(r.score[b, c]), cases.score_bound(int(r.n_views_of[c]))
        worst = max(worst, abs(float(score[b, c]) - want) / (bound * want) if want > 0 else float(score[b, c] != 0.0))
        assert abs(float(score[b, c]) - want) <= bound * want, (b, c, float(score[b, c]), want)
    assert np.isnan(score[r.is_match == 0]).all()
    n_views = int(r.n_views_of.sum())
    assert store.stats().last_round_upload_bytes == store_cases.upload_bytes(len(case["feat_id"]), len(case["box_corners"]), len(cand_owner), n_views)
    print("%d features, %d boxes, %d candidates, %d views: %d matches, largest score error %.2f of its bound" %
          (len(case["feat_id"]), len(case["box_corners"]), len(cand_owner), n_views, int(r.is_match.sum()), worst))
    return case, r, (in_box, count, overlap, match, score)


def load(store, model, case, seed):
    """The views of a case of cases.make_case into fresh owners of the store and the model, under scrambled keys, one put_views in upload order.  Returns the
    owners."""
    keys = store_cases.load_plan(case, seed)
    owners = [int(o) for o in store.new_owners(len(case["views"]))]
    assert owners == model.new_owners(len(case["views"]))
    flat = [(owners[c], k[0], k[1], ids) for c, views in enumerate(case["views"]) for k, ids in zip(keys[c], views)]
    args = [[f[0] for f in flat], [f[1] for f in flat], [f[2] for f in flat], [f[3] for f in flat]]
    store.put_views(*args)
    model.put_views(*args)
    return owners


def parity(ba, make_store, case, seed, listed=None):
    store, model = make_store(), store_cases.Model()
    owners = load(store, model, case, seed)
    same_state(store, model)
    listed = list(range(len(owners))) if listed is None else listed
    frame = {k: case[k] for k in ("feat_id", "feat_pixel", "box_corners", "box_label", "inflation", "min_overlap")}
    return check_round(ba, store, model, frame, [owners[c] for c in listed], [case["cand_label"][c] for c in listed])


MIXED = [[3, 10], [], [20, 1, 7], [5], [], [12, 12, 2]]


# ---- parity with the stateless entry and the restatement -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_feat", [0, 1, 63, 64, 65, 200])
def test_the_number_of_frame_features(ba, make_store, n_feat):
    _, r, _ = parity(ba, make_store, cases.make_case(100 + n_feat, n_feat, 5, MIXED), 1)
    assert n_feat < 63 or (r.overlap.sum() > 0 and r.count.max() > 0)


@pytest.mark.parametrize("offset", [-1, 0, 1])
def test_both_sides_of_the_lds_staging_limit(ba, make_store, offset):
    _, r, _ = parity(ba, make_store, cases.make_case(200 + offset, lds_limit() + offset, 3, [[40, 64, 5], [129], [], [12]], n_labels=1), 2)
    assert r.overlap.sum() > 0 and r.is_match.sum() > 0


@pytest.mark.parametrize("n_box", [0, 1, 63, 64, 65])
def test_the_number_of_boxes_around_the_bit_row_word(ba, make_store, n_box):
    _, r, _ = parity(ba, make_store, cases.make_case(400 + n_box, 100, n_box, MIXED), 3)
    assert n_box == 0 or r.overlap.sum() > 0
    if n_box == 65:
        assert r.count[64] > 0 and r.overlap[64].sum() > 0


def test_view_sizes_around_the_wavefront_within_one_call(ba, make_store):
    _, r, _ = parity(ba, make_store, cases.make_case(300, 200, 4, [[0, 1, 63], [64, 65, 129], [129, 0], [0]], n_labels=1), 4)
    assert (r.overlap.max(axis=0) > 0).sum() >= 4


def mixed_candidates(n_cand, rng):
    """Candidates of 0, 1 and 70 views in turn, the first and the last without views."""
    sizes = []
    for c in range(n_cand):
        n_views = 0 if c in (0, n_cand - 1) else (70, 1, 0)[c % 3]
        sizes.append([int(s) for s in rng.integers(0, 7, n_views)])
    return sizes


@pytest.mark.parametrize("which", ["none", "one_without_views", "65_mixed", "subset_in_reverse"])
def test_the_candidates_their_empty_view_ranges_and_their_order(ba, make_store, which):
    rng = np.random.default_rng(77)
    sizes = {"none": [], "one_without_views": [[]], "65_mixed": mixed_candidates(65, rng), "subset_in_reverse": mixed_candidates(11, rng)}[which]
    case = cases.make_case(500 + len(sizes), 120, 4, sizes, n_labels=1, min_overlap=1.0)
    listed = [10, 9, 8, 4, 3, 0] if which == "subset_in_reverse" else None        # a strict subset of the owners, in reverse order: 0, 70, 0, 1, 70 and 0 views
    _, r, _ = parity(ba, make_store, case, 5, listed)
    if which == "65_mixed":
        assert [len(s) for s in sizes[:4]] == [0, 1, 0, 70] and len(sizes[-1]) == 0 and r.is_match.sum() > 0 and r.is_match[:, [0, 64]].sum() == 0
    if which == "subset_in_reverse":
        assert list(r.n_views_of) == [0, 70, 0, 1, 70, 0] and r.is_match.sum() > 0


# ---- commit -------------------------------------------------------------------------------------------------------------------------------------------------------
def line_frame(seed, n_feat=400):
    """Features on a line, two pixels apart, under ids that are not sorted and reach above 2^32 and 2^63; boxes that hold exactly 0, 1, 63, 64, 65 and 130 of them
    and a seventh that holds 64 again."""
    rng = np.random.default_rng(seed)
    ids = cases.id_pool(rng, n_feat)
    assert ids != sorted(ids) and max(ids) >= cases.TOP and any((1 << 32) < i < cases.TOP for i in ids)
    pixel = np.stack([10.0 + 2.0 * np.arange(n_feat), np.full(n_feat, 100.0)], axis=1)
    spans = [None, (0, 0), (1, 63), (64, 127), (128, 192), (193, 322), (300, 363)]
    corners = [[0.0, 5.0, 300.0, 310.0] if s is None else [10.0 + 2.0 * s[0] - 0.5, 10.0 + 2.0 * s[1] + 0.5, 90.0, 110.0] for s in spans]
    order = rng.permutation(n_feat)                                                   # the caller's order is not the order along the line either
    return dict(feat_id=[ids[i] for i in order], feat_pixel=pixel[order], box_corners=np.array(corners), box_label=[0] * 7, inflation=0.0, min_overlap=2.0), [0, 1, 63, 64, 65, 130, 64]


def test_a_commit_stores_the_features_of_each_box_in_the_callers_order(ba, make_store):
    store, model = make_store(initial_pool_ids=256), store_cases.Model(256)
    frame, sizes = line_frame(11)
    owners = [int(o) for o in store.new_owners(6)]
    model.new_owners(6)
    _, r, _ = check_round(ba, store, model, frame, owners, [0] * 6)
    assert list(r.count) == sizes
    box_owner = owners + [-1]                                                         # the seventh box leaves no view
    store.commit(5, 1, box_owner)
    model.commit(5, 1, box_owner, store_cases.features_in_boxes(frame, r))
    same_state(store, model)
    assert [len(store.views(o)[0][1]) for o in owners] == sizes[:6] and store.stats().pool_growths == 1
    # a second round, on a frame that shares a part of the line, against the committed views -- the empty one among them counts in no score but exists
    again, _ = line_frame(12)
    again["feat_id"] = frame["feat_id"][:250] + again["feat_id"][250:]
    assert len(set(again["feat_id"])) == 400
    _, r2, _ = check_round(ba, store, model, again, owners[::-1], [0] * 6)
    assert r2.is_match.sum() > 0
    store.commit(6, 0, [owners[5], -1, -1, owners[0], -1, -1, -1])
    model.commit(6, 0, [owners[5], -1, -1, owners[0], -1, -1, -1], store_cases.features_in_boxes(again, r2))
    same_state(store, model)
    assert [k for k, _ in store.views(owners[0])] == [(5, 1), (6, 0)]


def test_a_frame_without_features_leaves_empty_views_that_count_in_the_next_divisor(ba, make_store):
    store, model = make_store(), store_cases.Model()
    a, b = [int(o) for o in store.new_owners(2)]
    model.new_owners(2)
    store.put_views([a, b], [2, 2], [0, 0], [[1, 2, 3, 4], [1, 2, 3, 4]])
    model.put_views([a, b], [2, 2], [0, 0], [[1, 2, 3, 4], [1, 2, 3, 4]])
    empty = dict(feat_id=[], feat_pixel=np.zeros((0, 2)), box_corners=[[0.0, 100.0, 0.0, 100.0], [50.0, 90.0, 50.0, 90.0]], box_label=[0, 0], inflation=0.0, min_overlap=1.0)
    _, r, _ = check_round(ba, store, model, empty, [a, b], [0, 0])
    assert r.is_match.sum() == 0
    store.commit(3, 0, [a, -1])
    model.commit(3, 0, [a, -1], [[], []])
    same_state(store, model)
    assert store.views(a) == [((2, 0), [1, 2, 3, 4]), ((3, 0), [])]
    frame = dict(feat_id=[4, 3, 2, 1], feat_pixel=[[10.0, 10.0]] * 4, box_corners=[[0.0, 100.0, 0.0, 100.0]], box_label=[0], inflation=0.0, min_overlap=1.0)
    _, _, (_, _, _, match, score) = check_round(ba, store, model, frame, [a, b], [0, 0])
    assert list(match[0]) == [1, 1] and score[0, 0] == 0.5 and score[0, 1] == 1.0      # the same view, once beside an empty one


# ---- replace, merge, release, window ---------------------------------------------------------------------------------------------------------------------------------
def both(store, model, name, *args):
    got, want = getattr(store, name)(*args), getattr(model, name)(*args)
    same_state(store, model, name)
    return got, want


def test_replace_merge_release_and_the_window(ba, make_store):
    store, model = make_store(), store_cases.Model()
    a, b, c, d = [int(o) for o in both(store, model, "new_owners", 4)[0]]
    both(store, model, "put_views", [a, a, b, b, c], [7, 3, 7, 5, 9], [0, 1, 0, 0, 2], [[1, 2, 3], [4], [5, 6], [7, 8, 9], [10]])
    both(store, model, "put_views", [a], [7], [0], [[11, 12, 13, 14]])                 # onto an existing key
    st = store.stats()
    assert st.replaced_views == 1 and st.dead_ids == 3 and st.live_ids == 11 and store.views(a) == [((3, 1), [4]), ((7, 0), [11, 12, 13, 14])]
    # a commit onto an existing key
    frame = dict(feat_id=[21, 22], feat_pixel=[[10.0, 10.0], [500.0, 10.0]], box_corners=[[0.0, 100.0, 0.0, 100.0]], box_label=[0], inflation=0.0, min_overlap=1.0)
    _, r, _ = check_round(ba, store, model, frame, [b, a], [0, 0])
    store.commit(5, 0, [b])
    model.commit(5, 0, [b], store_cases.features_in_boxes(frame, r))
    same_state(store, model, "commit")
    st = store.stats()
    assert st.replaced_views == 2 and st.dead_ids == 6 and store.views(b) == [((5, 0), [21]), ((7, 0), [5, 6])]
    # merge: from wins on the shared key (7, 0), its other key goes between into's
    both(store, model, "merge", [a], [b])
    assert store.views(b) == [((3, 1), [4]), ((5, 0), [21]), ((7, 0), [11, 12, 13, 14])] and store.stats().replaced_views == 2
    with pytest.raises(obvi_ba.ObviError):
        store.views(a)
    # a chain in one call: from[1] is into[0]
    both(store, model, "put_views", [d], [9], [2], [[30, 31]])
    both(store, model, "merge", [c, d], [d, b])
    assert store.views(b)[-1] == ((9, 2), [10]) and store.stats().owners == 1
    # the window: view_frame + window == frame_id stays, one below goes
    assert both(store, model, "apply_window", 9, 6) == (0, 0)
    assert both(store, model, "apply_window", 9, 5) == (1, 1) and [k for k, _ in store.views(b)] == [(5, 0), (7, 0), (9, 2)]
    # the wrap: INT_MIN in an unsigned frame id; frames below 2^31 give a huge sum, frames from 2^31 on wrap to a small one
    wrap = (1 << 64) - (1 << 31)
    e, = [int(o) for o in both(store, model, "new_owners", 1)[0]]
    both(store, model, "put_views", [e, e], [(1 << 31) + 4, (1 << 31) - 1], [0, 0], [[1], [2]])
    assert both(store, model, "apply_window", 9, wrap) == (1, 1) and [k for k, _ in store.views(e)] == [((1 << 31) - 1, 0)]
    assert both(store, model, "apply_window", 4, wrap) == (0, 0)                        # what is left sums to 2^64 - 1 or far above 4
    both(store, model, "release", [b])
    assert store.stats().owners == 1 and store.stats().views == 1
    both(store, model, "compact")
    assert store.stats().dead_ids == 0 and store.views(e) == [(((1 << 31) - 1, 0), [2])]


# ---- growth and compaction -----------------------------------------------------------------------------------------------------------------------------------------
def play(ba, store, ops, collect=None):
    """The session on a store: every call's outcome, and after every call the views of every owner and the stats, against the model.  `ba`: the scores are also
    held byte for byte against the stateless entry on that handle.  `collect` receives the bytes of everything read."""
    for i, op in enumerate(ops):
        what = "op %d %s" % (i, op.kind)
        if op.kind == "associate":
            out = store.associate(op.frame["feat_id"], op.frame["feat_pixel"], op.frame["box_corners"], op.frame["box_label"], op.cand_owner, op.cand_label, params_of(op.frame))
            r = op.restated
            assert all(np.array_equal(g, w) for g, w in zip(out[:4], (r.in_box, r.count, r.overlap, r.is_match))), what
            if ba is not None:
                stateless = ba.bbox_associate(*cases.arrays(op.case), params=params_of(op.frame))
                assert out[4].tobytes() == stateless[4].tobytes(), what
            for b, c in zip(*np.nonzero(r.is_match)):
                assert abs(float(out[4][b, c]) - float(r.score[b, c])) <= cases.score_bound(int(r.n_views_of[c])) * float(r.score[b, c]), what
            if collect is not None:
                collect.append(b"".join(x.tobytes() for x in out))
        elif op.kind == "new_owners":
            assert [int(o) for o in store.new_owners(op.n)] == op.want, what
        elif op.kind == "commit":
            store.commit(op.frame_id, op.camera_id, op.box_owner)
        elif op.kind == "merge":
            store.merge(op.from_owner, op.into_owner)
        elif op.kind == "release":
            store.release(op.owner)
        elif op.kind == "window":
            assert store.apply_window(op.frame_id, op.window) == op.dropped, what
        views, stats = op.after
        st = store.stats()
        assert {k: getattr(st, k) for k in store_cases.STATS} == stats, what
        got = {o: store.views(o) for o in views}
        assert got == views, what
        if collect is not None:
            collect.append(repr(got).encode())


def test_growth_and_compaction_follow_the_documented_rule_through_a_session(ba, make_store):
    ops = store_cases.session()
    facts = store_cases.session_facts(ops)
    assert facts["growths"] >= 2 and facts["compactions"] >= 2 and facts["compacted_before_associate"] and facts["replaced"] >= 1 and facts["empty_view"] and facts["apart"]
    store = make_store(initial_pool_ids=store_cases.SESSION_POOL, compact_min_dead_ids=store_cases.SESSION_MIN_DEAD)
    play(ba, store, ops)
    st = store.stats()
    assert st.pool_growths == facts["growths"] and st.compactions == facts["compactions"]
    print("session: %d calls, %d growths to %d ids, %d compactions, %d replaced views" % (len(ops), st.pool_growths, st.pool_capacity_ids, st.compactions, st.replaced_views))


def test_default_and_deterministic_handles_give_the_same_bytes(ba, make_store):
    ops = store_cases.session()[:60]
    det = helpers.product_ba(deterministic=True)
    det_store = obvi_ba.BboxStore(det, initial_pool_ids=64, compact_min_dead_ids=1)
    try:
        a, b = [], []
        play(None, make_store(initial_pool_ids=64, compact_min_dead_ids=1), ops, a)
        play(None, det_store, ops, b)
    finally:
        det_store.close()                                                             # the store before its handle
        det.close()
    assert a == b and len(a) > 60


# ---- upload size ---------------------------------------------------------------------------------------------------------------------------------------------------
def test_a_round_uploads_the_same_bytes_whatever_the_views_hold(ba, make_store):
    rng = np.random.default_rng(9)
    keys = [(int(f), int(c)) for f, c in zip(rng.integers(0, 50, 24), rng.integers(0, 1 << 40, 24))]
    frame = cases.make_case(900, 150, 4, [])
    frame = {k: frame[k] for k in ("feat_id", "feat_pixel", "box_corners", "box_label", "inflation", "min_overlap")}
    sent = []
    for scale in (1, 10):
        store, model = make_store(), store_cases.Model()
        owners = [int(o) for o in store.new_owners(6)]
        model.new_owners(6)
        views = [frame["feat_id"][k:k + 3] + [(1 << 34) + 1000 * k + j for j in range(scale * (3 + k % 5) - 3)] for k in range(24)]
        args = [[owners[k % 5] for k in range(24)], [k[0] for k in keys], [k[1] for k in keys], views]      # the sixth owner has no views
        store.put_views(*args)
        model.put_views(*args)
        check_round(ba, store, model, frame, owners, [0, 1, 0, 1, 0, 1])
        sent.append((store.stats().last_round_upload_bytes, store.stats().live_ids))
    assert sent[0][0] == sent[1][0] == 32 * 150 + 36 * 4 + 4 * 6 + 8 * 7 + 16 * 24 and sent[1][1] == 10 * sent[0][1]


# ---- refusals on a live store ----------------------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_store_as_it_was(ba, make_store):
    store, model = make_store(), store_cases.Model()
    a, b, gone = [int(o) for o in store.new_owners(3)]
    model.new_owners(3)
    both(store, model, "put_views", [a, b, gone], [1, 1, 1], [0, 0, 0], [[1, 2], [3], [4]])
    both(store, model, "release", [gone])
    frame = dict(feat_id=[1, 2, 3], feat_pixel=[[10.0, 10.0]] * 3, box_corners=[[0.0, 100.0, 0.0, 100.0]], box_label=[0], inflation=0.0, min_overlap=1.0)
    last_error = ba._lib.obvi_ba_last_error
    last_error.restype = C.c_char_p

    def refused(status, fn, *args, **kw):
        with pytest.raises(obvi_ba.ObviError, match="status %d " % status):
            fn(*args, **kw)
        assert b"bbox store" in last_error(ba._h)
        same_state(store, model, fn.__name__)

    def associate(**change):
        f = dict(frame, **{k: v for k, v in change.items() if k in frame})
        return store.associate(f["feat_id"], f["feat_pixel"], f["box_corners"], f["box_label"], change.get("cand", [a, b]), change.get("labels", [0, 0]), params_of(f))

    refused(INVALID, store.commit, 2, 0, [a])                                          # no round is kept
    for owner in (gone, 99, -5):                                                       # released, unknown
        refused(INVALID, store.put_views, [owner], [2], [0], [[7]])
        refused(INVALID, associate, cand=[a, owner])
        refused(INVALID, store.merge, [owner], [a])
        refused(INVALID, store.merge, [a], [owner])
        refused(INVALID, store.release, [a, owner])
        refused(INVALID, store.views, owner)
    refused(INVALID, associate, cand=[a, a])
    refused(INVALID, store.merge, [a], [a])
    refused(INVALID, store.merge, [a, a], [b, b])                                      # released earlier in the same list
    refused(INVALID, store.release, [a, a])
    refused(INVALID, store.put_views, [a], [2], [0], [[7, 8, 7]])                      # an id twice in a view
    refused(INVALID, store.put_views, [a, a], [2, 2], [0, 0], [[7], [8]])              # the same view twice in a call
    refused(NUMERICAL, associate, box_corners=[[0.0, np.nan, 0.0, 100.0]])
    refused(NUMERICAL, associate, box_corners=[[0.0, 100.0, -np.inf, 100.0]])
    refused(INVALID, associate, feat_id=[1, 2, 1])                                     # a frame id twice
    # around a kept round: a refused associate leaves it kept; commit takes it once
    associate()
    refused(INVALID, associate, cand=[a, gone])
    refused(INVALID, store.commit, 2, 0, [a, b])                                       # another n_box
    refused(INVALID, store.commit, 2, 0, [gone])
    refused(INVALID, store.commit, 2, 0, [77])
    associate(box_corners=[[0.0, 100.0, 0.0, 100.0], [0.0, 50.0, 0.0, 50.0]], box_label=[0, 0])
    refused(INVALID, store.commit, 2, 0, [a, a])                                       # an owner twice
    store.commit(2, 0, [a, -1])
    model.commit(2, 0, [a, -1], [[1, 2, 3], [1, 2, 3]])
    same_state(store, model)
    refused(INVALID, store.commit, 2, 0, [a, -1])                                      # commit twice
    assert store.views(a) == [((1, 0), [1, 2]), ((2, 0), [1, 2, 3])]
