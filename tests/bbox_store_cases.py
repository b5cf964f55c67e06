"""Support of tests/test_bbox_store_abi.py and tests/test_gpu_bbox_store.py: a model of the appearance store (include/obvi_bbox_store.h) and the session it is
run through.

The model is a dict of dicts, owner -> {(frame, camera): [ids]}, plus the counters the header documents: the pool grows by doubling until an append fits (one
growth per reallocation), and after every mutating call the pool is compacted when dead_ids >= compact_min_dead_ids and dead_ids > live_ids.  It holds no offsets
and shares no code with the library.  The round itself is judged by the restatement of tests/bbox_frontend_cases.py, over the model's views in (frame, camera)
order."""
import copy
import functools

import numpy as np

import bbox_frontend_cases as cases

MASK = (1 << 64) - 1
STATS = ("owners", "views", "live_ids", "dead_ids", "pool_capacity_ids", "pool_growths", "compactions", "replaced_views")


class Model:
    def __init__(self, initial_pool_ids=65536, compact_min_dead_ids=65536):
        self.owners, self.next_owner = {}, 0
        self.cap, self.min_dead = initial_pool_ids, compact_min_dead_ids
        self.live = self.dead = self.growths = self.compactions = self.replaced = 0

    # ---- the documented rules ------------------------------------------------------------------------------------------------------------------------------
    def _reserve(self, n):
        need = self.live + self.dead + n
        if need > self.cap:
            while self.cap < need:
                self.cap *= 2
            self.growths += 1

    def _compact_if_due(self):
        if self.dead >= self.min_dead and self.dead > self.live:
            self.compact()

    def compact(self):
        self.dead = 0
        self.compactions += 1

    def _place(self, owner, key, ids, count_replaced):
        views = self.owners[owner]
        if key in views:
            self.live -= len(views[key])
            self.dead += len(views[key])
            self.replaced += int(count_replaced)
        views[key] = list(ids)
        self.live += len(ids)

    # ---- the entries -----------------------------------------------------------------------------------------------------------------------------------------
    def new_owners(self, n):
        out = list(range(self.next_owner, self.next_owner + n))
        for o in out:
            self.owners[o] = {}
        self.next_owner += n
        return out

    def put_views(self, owner, frame, camera, views):
        self._reserve(sum(len(v) for v in views))
        for o, f, c, ids in zip(owner, frame, camera, views):
            self._place(int(o), (int(f), int(c)), ids, True)
        self._compact_if_due()

    def commit(self, frame_id, camera_id, box_owner, features_in_bb):
        taking = [(int(o), ids) for o, ids in zip(box_owner, features_in_bb) if int(o) != -1]
        self._reserve(sum(len(ids) for _, ids in taking))
        for o, ids in taking:
            self._place(o, (int(frame_id), int(camera_id)), ids, True)
        self._compact_if_due()

    def merge(self, from_owner, into_owner):
        for f, t in zip(from_owner, into_owner):
            for key, ids in self.owners[f].items():
                self.live -= len(ids)                                                # the view changes hands; what it lands on dies
                self._place(t, key, ids, False)
            del self.owners[f]
        self._compact_if_due()

    def release(self, owner):
        for o in owner:
            n = sum(len(ids) for ids in self.owners[o].values())
            self.live -= n
            self.dead += n
            del self.owners[o]
        self._compact_if_due()

    def apply_window(self, frame_id, window):
        dropped = 0
        for views in self.owners.values():
            for key in [k for k in views if ((k[0] + window) & MASK) < frame_id]:
                self.live -= len(views[key])
                self.dead += len(views[key])
                del views[key]
                dropped += 1
        self._compact_if_due()
        return dropped

    # ---- what the tests compare --------------------------------------------------------------------------------------------------------------------------------
    def views(self, owner):
        return [(key, list(self.owners[owner][key])) for key in sorted(self.owners[owner])]

    def stats(self):
        return dict(owners=len(self.owners), views=sum(len(v) for v in self.owners.values()), live_ids=self.live, dead_ids=self.dead, pool_capacity_ids=self.cap,
                    pool_growths=self.growths, compactions=self.compactions, replaced_views=self.replaced)

    def snapshot(self):
        return {o: self.views(o) for o in self.owners}, self.stats()


def round_case(model, frame, cand_owner, cand_label):
    """The case of bbox_frontend_cases (restate, arrays) for a frame -- feat_id, feat_pixel, box_corners, box_label, inflation, min_overlap -- against the stored
    views of the listed owners, in (frame, camera) order."""
    return dict(frame, cand_label=[int(x) for x in cand_label], views=[[ids for _, ids in model.views(int(o))] for o in cand_owner])


def features_in_boxes(frame, r):
    """Per box the ids of the restated round's features inside it, in the caller's feature order: features_in_bb of the host path."""
    return [[fid for i, fid in enumerate(frame["feat_id"]) if r.in_box[b, i]] for b in range(len(frame["box_corners"]))]


def upload_bytes(n_feat, n_box, n_cand, n_views):
    """last_round_upload_bytes as the header states it."""
    return 0 if n_box == 0 else 32 * n_feat + 36 * n_box + 4 * n_cand + 8 * (n_cand + 1) + 16 * n_views


def scrambled_keys(rng, n):
    """n distinct (frame, camera) keys in an order that is not the sorted one; frames below 2^20, above 2^32 and above 2^63, cameras 0..2."""
    keys = set()
    while len(keys) < n:
        f = int(rng.integers(0, 1 << 20))
        keys.add(((f, (f << 32) | 7, f | cases.TOP)[int(rng.integers(3))], int(rng.integers(3))))
    keys = list(keys)
    keys = [keys[i] for i in rng.permutation(n)]
    if n > 1 and keys == sorted(keys):
        keys[0], keys[-1] = keys[-1], keys[0]
    return keys


def load_plan(case, seed):
    """For a case of bbox_frontend_cases.make_case: per candidate the keys of its views, in upload order."""
    rng = np.random.default_rng(seed)
    return [scrambled_keys(rng, len(views)) for views in case["views"]]


# ---- the session of the growth and compaction test ---------------------------------------------------------------------------------------------------------------
SESSION_SEED = 4
SESSION_POOL, SESSION_MIN_DEAD = 64, 1
SESSION_ROUNDS, SESSION_WINDOW = 40, 5


class Op:
    """One call on the store and the model's state after it.  kind: new_owners, associate, commit, merge, release, window."""

    def __init__(self, kind, **kw):
        self.kind = kind
        self.__dict__.update(kw)


@functools.lru_cache(maxsize=None)
def session(seed=SESSION_SEED):
    """About 40 rounds over a fixed scene of 300 features and five places where boxes appear, one of them where no feature lies (its views are empty).  A frame
    sees about 130 of the features and three of the boxes; a box goes to the owner the restated round and the greedy rule give it, or opens one.  Some rounds
    come again under the key of the round before (the views are replaced), one box in five leaves no view, and merges, releases and the validity window are
    mixed in.  Returns the list of Ops; every Op carries the model's snapshot after it."""
    rng = np.random.default_rng(seed)
    world_id = cases.id_pool(rng, 300)
    world_px = np.round(rng.uniform([0, 0], [640, 400], (300, 2)) * 4) / 4              # nothing below y = 400: the fifth place is empty
    places = np.array([[40.0, 200.0, 30.0, 150.0], [230.0, 420.0, 60.0, 200.0], [400.0, 620.0, 180.0, 380.0], [60.0, 260.0, 220.0, 390.0], [300.0, 400.0, 420.0, 470.0]])
    place_label = [0, 1, 0, 1, 0]
    model = Model(SESSION_POOL, SESSION_MIN_DEAD)
    label_of, ops = {}, []
    frame_id = 0

    def done(op):
        op.after = copy.deepcopy(model.snapshot())
        ops.append(op)

    for rnd in range(SESSION_ROUNDS):
        again = rnd % 6 == 4                                                            # this round comes under the key of the one before
        if not again:
            frame_id += 1
        camera_id = (frame_id % 2)
        seen = np.sort(rng.choice(300, size=int(rng.integers(120, 141)), replace=False))
        seen = seen[rng.permutation(len(seen))]
        which = sorted(rng.choice(5, size=3, replace=False).tolist()) if rnd % 4 else [0, 2, 4]
        corners = places[which] + np.round(rng.uniform(-4, 4, (3, 4)) * 4) / 4
        frame = dict(feat_id=[world_id[i] for i in seen], feat_pixel=world_px[seen], box_corners=corners, box_label=[place_label[p] for p in which], inflation=2.5,
                     min_overlap=2.0)
        cand = sorted(model.owners)
        if rnd % 3 == 1:
            cand = cand[::-1]
        case = round_case(model, frame, cand, [label_of[o] for o in cand])
        r = cases.restate(case)
        done(Op("associate", frame=frame, cand_owner=cand, cand_label=case["cand_label"], case=case, restated=r, apart=cases.competing_scores_are_apart(r, 100.0)))
        box_owner = []
        for b, (new, c) in enumerate(cases.assign_restated(r, len(cand))):
            if new:
                o = model.new_owners(1)[0]
                label_of[o] = frame["box_label"][b]
                done(Op("new_owners", n=1, want=[o]))
                box_owner.append(o)
            else:
                box_owner.append(cand[c])
        if rnd % 5 == 3:
            box_owner[1] = -1
        model.commit(frame_id, camera_id, box_owner, features_in_boxes(frame, r))
        done(Op("commit", frame_id=frame_id, camera_id=camera_id, box_owner=box_owner))
        if rnd % 7 == 5:
            by_label = {}
            for o in sorted(model.owners):
                by_label.setdefault(label_of[o], []).append(o)
            pairs = [v for v in by_label.values() if len(v) >= 3]
            if pairs:
                a, b, c = pairs[0][-1], pairs[0][-2], pairs[0][0]                        # a chain: a into b, then b into c
                model.merge([a, b], [b, c])
                done(Op("merge", from_owner=[a, b], into_owner=[b, c]))
        if rnd % 9 == 8:
            gone = sorted(model.owners)[:2]
            model.release(gone)
            done(Op("release", owner=gone))
        if rnd % 2 == 1:
            dropped = model.apply_window(frame_id, SESSION_WINDOW)
            done(Op("window", frame_id=frame_id, window=SESSION_WINDOW, dropped=dropped))
    return ops


def session_facts(ops):
    """What the chosen seed must show, from the model alone."""
    stats = [op.after[1] for op in ops]
    compacted_before_associate = any(ops[i + 1].kind == "associate" and stats[i]["compactions"] > (stats[i - 1]["compactions"] if i else 0) for i in range(len(ops) - 1))
    empty_view = any(len(ids) == 0 for op in ops for views in op.after[0].values() for _, ids in views)
    return dict(growths=stats[-1]["pool_growths"], compactions=stats[-1]["compactions"], replaced=stats[-1]["replaced_views"], empty_view=empty_view,
                compacted_before_associate=compacted_before_associate, apart=all(op.apart for op in ops if op.kind == "associate"),
                rounds=sum(op.kind == "associate" for op in ops), kinds=sorted(set(op.kind for op in ops)),
                matches=sum(int(op.restated.is_match.sum()) for op in ops if op.kind == "associate"))
