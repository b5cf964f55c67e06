"""GPU (-m gpu): the device-resident map and CONCURRENT sessions together (include/obvi_map_shared.h): joint map priors (types 9 and 10) on
handles that exchange shared objects, and the joint posterior folded back into a map by every member through the handle forms.

Shape: four sessions of 60 frames / 900 features over TEN shared objects -- the smallest count whose tail crosses the 64-row tile edge (od 7: 70 rows, two tail
tile rows; od 9: 90 rows); a 70-row group is two slabs of the quad kernel and three scatter tiles, and some object's block straddles row 64.

Yardstick for everything linear -- never the product: Sigma_ref = inv(S_oracle(radius 1e300) + scatter(w Lambda)), numpy on the CPU oracle's joint reduced
system of synth.join_problems(sessions) at the members' state, Lambda = C^-1 from long double, w from the Huber rule at that state.  Bar: 1e-7 of a block's
largest entry, the bar tests/test_gpu_joint_covariance.py sets for a joint system of this size.  LM trajectories: the bars of
test_gpu_session_groups.check_member_against_joint (same decisions, costs 1e-8, poses 1e-8, objects 1e-7).  The update of the handle forms: 1e-11 against
numpy's evaluation of the update formulas fed the product's own posterior (the bar of tests/test_gpu_map_update.py / test_gpu_map_extend.py), bit-equality against
the host-pointer forms on deterministic handles."""
import ctypes as C
import types

import numpy as np
import pytest
import torch

import dist_util
import helpers
import map_extend_cases
import map_update_cases
import obvi_ba
import synth
import test_gpu_covariance_blocks as blocks
import test_gpu_session_groups as groups
from test_gpu_joint_covariance import GROUP_TIMEOUT, collective, member_states, open_job, solve_job, statuses
from test_gpu_map_pair_priors import base_problem, inv_ld, product, spd

pytestmark = pytest.mark.gpu

POSE, OBJ = blocks.POSE, blocks.OBJ
BAR = 1e-7
LD = np.longdouble
T = obvi_ba.FACTOR_MAP_GROUP_PRIOR
N_OBJ = 10
IDS = np.arange(N_OBJ, dtype=np.uint32)
SESSIONS = dict(groups.SESSIONS, O=N_OBJ, const_poses=1)


@pytest.fixture(scope="module")
def sessions():
    return synth.make_sessions(**SESSIONS)


def of_block_size(sessions, od):
    return [synth.nine_dof(q) for q in sessions] if od == 9 else sessions


def close_job(group, handles):
    for ba in handles:
        ba.close()
    group.close()


def open_shared_job(sessions, od=7, deterministic=False):
    """open_job with the collective form of the map entries switched on for every member"""
    group, handles = open_job(sessions, od, deterministic)
    for h in handles:
        h.map_allow_exchange(True)
    return group, handles


# ---- the priors ----------------------------------------------------------------------------------------------------------------------------------------
def the_prior(objects, od, dense, seed=41):
    """(mean [n][od], C [n od][n od]) beside the objects' start estimates: dense C = spd(cond 1e3), or block diagonal with spd blocks"""
    rng = np.random.default_rng(seed)
    n = len(objects)
    mean = objects - rng.normal(scale=0.02, size=(n, od))
    if dense:
        cov = spd(rng, n * od)
    else:
        cov = np.zeros((n * od, n * od))
        for o in range(n):
            cov[od * o:od * o + od, od * o:od * o + od] = spd(rng, od)
    return mean, cov


def huber_of(prior, objects, huber):
    """(s, w, rho) of one group prior (members, mean, cov) at `objects`, long double"""
    members, mean, cov = prior
    L = inv_ld(cov)
    d = (objects[list(members)] - mean).ravel().astype(LD)
    s = float(d @ L @ d)
    w = 1.0 if s <= huber * huber else huber / np.sqrt(s)
    rho = s if s <= huber * huber else 2.0 * huber * np.sqrt(s) - huber * huber
    return s, w, rho


class Reference:
    """The oracle's joint reduced system at a state, plus w Lambda of the group priors on the object rows: Sigma_ref."""

    def __init__(self, joint, od, priors, huber, times=1):
        self.od, self.joint = od, joint
        self.o = o = helpers.oracle_ba(object_block_size=od)
        synth.upload(o, joint)
        self.pvar, self.lvar, self.ovar = blocks.parameters(o)
        self.prow, self.orow = blocks.canonical(self.pvar, self.ovar, od)
        S, _ = o.debug_reduced_system(1e300)
        assert S.shape[0] == 6 * self.pvar.sum() + od * self.ovar.sum()
        S = np.array(S)
        self.w = []
        for prior in priors:
            members = list(prior[0])
            _, w, _ = huber_of(prior, joint["objects"], huber)
            rows = np.concatenate([np.arange(self.orow[m], self.orow[m] + od) for m in members])
            S[np.ix_(rows, rows)] += times * w * inv_ld(prior[2]).astype(np.float64)
            self.w.append(w)
        self.cond = float(np.linalg.cond(S))
        self.Sigma = np.linalg.inv(S)

    def obj_block(self, a, b):
        ra, rb = self.orow[a], self.orow[b]
        return self.Sigma[ra:ra + self.od, rb:rb + self.od]

    def obj_part(self, ids):
        rows = np.concatenate([np.arange(self.orow[i], self.orow[i] + self.od) for i in ids])
        return self.Sigma[np.ix_(rows, rows)]


def joint_at(sessions, states):
    joint = synth.join_problems(sessions)
    joint.update(poses=np.concatenate([s[0] for s in states]), points=np.concatenate([s[1] for s in states]), objects=states[0][2])
    return joint


def blocks_of(M, od):
    k = len(M) // od
    return M.reshape(k, od, k, od).transpose(0, 2, 1, 3)


def worst_block(got, want, od):
    """largest deviation of an od x od block relative to the wanted block's largest entry"""
    g, w = blocks_of(np.asarray(got), od), blocks_of(np.asarray(want), od)
    return max(blocks.block_err(g[a, b], w[a, b]) for a in range(g.shape[0]) for b in range(g.shape[1]))


def check_every_block(handles, sessions, ref, label, ids=IDS):
    """all shared x shared blocks of the merged route, and pose / shared-object / on-pattern cross blocks of the selected inversion, on every member"""
    od = ref.od
    a, b = np.array([(i, j) for i in ids for j in ids]).T
    merged = collective(handles, lambda m, h: h.object_covariances(a, b))
    e_merged = max(blocks.block_err(c[x], ref.obj_block(a[x], b[x])) for c in merged for x in range(len(a)))
    print("%s: %d shared x shared blocks per member from the merged route %.3e (bar %.0e), cond %.2e, w %s" % (label, len(a), e_merged, BAR, ref.cond, ref.w))
    collective(handles, lambda m, h: h.covariance_compute())
    po = ref.joint["session_pose_offsets"]
    worst = [e_merged]
    for s, (q, g) in enumerate(zip(sessions, handles)):
        prow = ref.prow[po[s]:po[s + 1]]
        cp = g.pose_covariances(np.arange(len(q["poses"])))
        e_pose = max(blocks.block_err(cp[p], ref.Sigma[prow[p]:prow[p] + 6, prow[p]:prow[p] + 6]) for p in range(len(prow)) if prow[p] >= 0)
        own = g.object_covariance_blocks(ids)
        e_own = max(blocks.block_err(own[x], ref.obj_block(i, i)) for x, i in enumerate(ids))
        rows = {(POSE, p): int(prow[p]) for p in range(len(prow)) if prow[p] >= 0}
        rows.update({(OBJ, int(i)): int(ref.orow[i]) for i in ids})
        dims = {k: (6 if k[0] == POSE else od) for k in rows}
        pairs = [pr for pr in blocks.joined_pairs(q, prow >= 0, ref.ovar) if pr[1][0] == OBJ and pr[1][1] in ids]
        pairs += [((OBJ, int(i)), (OBJ, int(j))) for i in ids for j in ids if i < j]          # coupled by the prior alone where no frame sees both
        ka, ia, kb, ib = zip(*[(x[0], x[1], y[0], y[1]) for x, y in pairs])
        assert g.covariance_on_pattern(ka, ia, kb, ib).all()
        print("%s member %d: pose blocks %.3e, shared blocks %.3e" % (label, s, e_pose, e_own))
        blocks.check_cross(g, pairs, rows, dims, ref.Sigma, BAR, "%s member %d" % (label, s))
        worst += [e_pose, e_own]
    assert max(worst) < BAR, worst
    return merged


def summary_dict(o):
    return dict(num_iterations=o.num_iterations, termination_type=o.termination_type, initial_cost=o.initial_cost, final_cost=o.final_cost)


def check_trajectory(ref, sessions, handles, out):
    for m, (o, ba) in enumerate(zip(out, handles)):
        groups.check_member_against_joint(ref, m, summary_dict(o), [(i.step_is_successful, i.cost) for i in ba.iterations()], ba.get_poses(), ba.get_points(), ba.get_objects())


def reference_run(ba, joint):
    """what check_member_against_joint reads, from a handle that solved the joint problem"""
    s = ba.solve(helpers.ba_params(max_it=15))
    return dict(joint=joint, summary=s, its=ba.iterations(), poses=ba.get_poses(), objects=ba.get_objects(), points=ba.get_points())


# ---- 1. the switch -------------------------------------------------------------------------------------------------------------------------------------
def test_switch_off_refuses_as_before_and_reset_clears_it():
    od = 7
    prob = base_problem(od)
    rng = np.random.default_rng(3)
    m = prob["objects"] + 0.01
    calls = []
    mean, cov = prob["objects"][:2], spd(rng, 2 * od)

    def exchanging():
        ex = product(prob)
        ex.set_map_group_priors([[0, 2]], [m[[0, 2]]], [spd(rng, 2 * od)])
        ex.set_shared_objects(np.array([0, 0, 1, 0, 0], np.uint8), 0, 1)
        ex.set_allreduce(lambda buf, count, op, stream: calls.append(count) or 0)
        return ex

    def refused(ex):
        for call in (ex.prepare, lambda: ex.solve(helpers.ba_params(max_it=2)), lambda: ex.evaluate(), ex.covariance_compute):
            with pytest.raises(obvi_ba.ObviError, match="status -1 map group priors on a handle that exchanges shared objects: the collective form is not built"):
                call()
        with obvi_ba.Map.create(mean, cov, library=helpers.PRODUCT_LIB) as mp:
            with pytest.raises(obvi_ba.ObviError, match="status -1 map_condition_on_handle: the handle exchanges shared objects"):
                mp.condition_on(ex, [0, 2], [0, 1])
            with pytest.raises(obvi_ba.ObviError, match="status -1 map_extend_on_handle: the handle exchanges shared objects"):
                mp.extend_on(ex, [0], [0], [2])
            with pytest.raises(obvi_ba.ObviError, match="status -1 map_extend_on_handle: the handle exchanges shared objects"):
                obvi_ba.Map.from_handle(ex, [0, 2])
    ex = exchanging()
    refused(ex)
    assert calls == []                                                                  # the hook was never called
    f = ex._lib.obvi_map_allow_exchange
    f.restype = C.c_int
    for bad in (2, -1, 7):
        assert f(ex._h, C.c_int32(bad)) == -1
    refused(ex)                                                                         # a refused value leaves the switch where it was
    ex.map_allow_exchange(True)
    ex.prepare()                                                                        # validated and planned: no collective yet
    assert calls == []
    ex.map_allow_exchange(False)
    refused(ex)                                                                         # off again: as before, with a plan in hand
    ex.map_allow_exchange(True)
    ex.reset()
    synth.upload(ex, prob)
    ex.set_map_group_priors([[0, 2]], [m[[0, 2]]], [spd(rng, 2 * od)])
    ex.set_shared_objects(np.array([0, 0, 1, 0, 0], np.uint8), 0, 1)
    ex.set_allreduce(lambda buf, count, op, stream: calls.append(count) or 0)
    refused(ex)                                                                         # obvi_ba_reset cleared the switch
    assert calls == []
    ex.close()


# ---- 2. block-diagonal priors are type-4 priors ------------------------------------------------------------------------------------------------------------
_type4_runs = {}


def type4_reference(sessions, od):
    """the ORACLE's LM run on the joint problem with ten independent (type-4) priors, once per block size"""
    if od not in _type4_runs:
        qs = of_block_size(sessions, od)
        mean, cov = the_prior(qs[0]["objects"], od, dense=False)
        first = dict(qs[0], lt_obj=IDS, lt_mean=mean, lt_cov=np.stack([cov[od * o:od * o + od, od * o:od * o + od].ravel() for o in range(N_OBJ)]), lt_huber=1e6)
        joint = synth.join_problems([first] + list(qs[1:]))
        orc = helpers.oracle_ba(object_block_size=od)
        synth.upload(orc, joint)
        s = orc.solve(helpers.ba_params(max_it=15))
        _type4_runs[od] = (qs, mean, cov, dict(joint=joint, summary=s, its=orc.iterations(), poses=orc.get_poses(), objects=orc.get_objects(), points=orc.get_points()))
    return _type4_runs[od]


@pytest.mark.parametrize("form,od,deterministic", [("group", 7, False), ("group", 9, False), ("group", 7, True), ("pairs", 7, False)])
def test_block_diagonal_priors_are_independent_priors_against_the_oracles_run(sessions, form, od, deterministic):
    qs, mean, cov, ref = type4_reference(sessions, od)
    group, handles = open_shared_job(qs, od, deterministic)
    try:
        if form == "group":
            handles[0].set_map_group_priors([list(IDS)], [mean], [cov], 1e6)
        else:
            a, b = IDS[0::2], IDS[1::2]
            cj = np.stack([cov[np.ix_(r, r)] for r in (np.concatenate([np.arange(od * x, od * x + od), np.arange(od * y, od * y + od)]) for x, y in zip(a, b))])
            handles[0].set_map_pair_priors(a, b, mean[a], mean[b], cj, None, 1e6)
        out = collective(handles, lambda m, h: h.solve(helpers.ba_params(max_it=15)))
        print("%s od %d deterministic %d: %d iterations, final cost %.9e (oracle %.9e)" % (form, od, deterministic, out[0].num_iterations, out[0].final_cost, ref["summary"].final_cost))
        check_trajectory(ref, qs, handles, out)
        for h in handles[1:]:
            assert np.array_equal(h.get_objects(), handles[0].get_objects())
    finally:
        close_job(group, handles)


# ---- 3. dense C, any member, every block ---------------------------------------------------------------------------------------------------------------------
def dense_job(sessions, od, deterministic, huber, uploaders=(2,)):
    mean, cov = the_prior(sessions[0]["objects"], od, dense=True)
    prior = (list(IDS), mean, cov)
    orc = helpers.oracle_ba(object_block_size=od)
    synth.upload(orc, synth.join_problems(sessions))
    cost0 = orc.evaluate()[0]
    group, handles = open_shared_job(sessions, od, deterministic)
    for u in uploaders:
        handles[u].set_map_group_priors([list(IDS)], [mean], [cov], huber)
    start = huber_of(prior, sessions[0]["objects"], huber)
    out = solve_job(handles)
    for o in out:
        want = cost0 + 0.5 * len(uploaders) * start[2]
        print("initial cost %.15e, oracle's joint cost + rho / 2 %.15e: %.2e (bar 1e-12)" % (o.initial_cost, want, abs(o.initial_cost - want) / want))
    assert all(abs(o.initial_cost - (cost0 + 0.5 * len(uploaders) * start[2])) <= 1e-12 * (cost0 + 0.5 * len(uploaders) * start[2]) for o in out)
    ref = Reference(joint_at(sessions, member_states(handles)), od, [prior], huber, times=len(uploaders))
    return types.SimpleNamespace(group=group, handles=handles, out=out, ref=ref, prior=prior, mean=mean, cov=cov, start=start, huber=huber)


@pytest.fixture(scope="module")
def solved(sessions):
    """Case 3's job on deterministic handles: member 2 uploads one dense group over the ten objects, w = 1; solved once, left where the solve ended.  Cases 8 to
    10 fold its posterior back: they linearise and never move the estimate."""
    job = dense_job(sessions, 7, True, 1e6)
    yield job
    close_job(job.group, job.handles)


def test_dense_prior_uploaded_by_member_two_every_block_on_every_member(sessions, solved):
    assert solved.start[1] == 1.0 and solved.ref.w == [1.0]
    check_every_block(solved.handles, sessions, solved.ref, "dense C, w = 1")


def test_dense_prior_with_a_huber_weight_below_one(sessions):
    huber = 0.5
    job = dense_job(sessions, 7, False, huber)
    try:
        print("s %.4e at the start: w %.4f;  at the solution: w %.4f" % (job.start[0], job.start[1], job.ref.w[0]))
        assert job.start[1] < 1.0
        check_every_block(job.handles, sessions, job.ref, "dense C, huber %.1f" % huber)
    finally:
        close_job(job.group, job.handles)


# ---- 4. trajectory with dense C ---------------------------------------------------------------------------------------------------------------------------------
def test_trajectory_follows_one_plain_handle_that_holds_the_joint_problem(sessions):
    od = 7
    mean, cov = the_prior(sessions[0]["objects"], od, dense=True)
    joint = synth.join_problems(sessions)
    plain = product(joint)
    plain.set_map_group_priors([list(IDS)], [mean], [cov], 2.0)
    ref = reference_run(plain, joint)
    plain.close()
    group, handles = open_shared_job(sessions, od)
    try:
        handles[2].set_map_group_priors([list(IDS)], [mean], [cov], 2.0)
        out = collective(handles, lambda m, h: h.solve(helpers.ba_params(max_it=15)))
        print("dense C, huber 2: %d iterations, final cost %.9e (one plain handle %.9e)" % (out[0].num_iterations, out[0].final_cost, ref["summary"].final_cost))
        assert out[0].num_iterations > 3
        check_trajectory(ref, sessions, handles, out)
    finally:
        close_job(group, handles)


# ---- 5. shared and private members in one group ---------------------------------------------------------------------------------------------------------------
def test_shared_and_private_members_in_one_group():
    od, O = 7, 12
    joint = synth.join_problems(synth.make_sessions(**dict(SESSIONS, O=O)))
    mean, cov = the_prior(joint["objects"], od, dense=True)
    members = list(range(O))
    runs = []
    for shared in (False, True):
        g = product(joint)
        g.set_map_group_priors([members], [mean], [cov], 1e6)
        if shared:
            flags = np.zeros(O, np.uint8); flags[:N_OBJ] = 1
            g.set_shared_objects(flags, 0, 1)
            g.set_allreduce(lambda ptr, n, op, stream: 0)
            g.map_allow_exchange(True)
        runs.append((g, reference_run(g, joint)))
    (plain, ref), (g, got) = runs
    s = got["summary"]
    print("twelve objects, ten shared: %d iterations, final cost %.9e (without shared flags %.9e)" % (s.num_iterations, s.final_cost, ref["summary"].final_cost))
    assert s.num_iterations > 3
    groups.check_member_against_joint(dict(ref, joint=dict(joint, session_pose_offsets=[0, len(joint["poses"])], session_point_offsets=[0, len(joint["points"])])), 0,
                                      summary_dict(s), [(i.step_is_successful, i.cost) for i in got["its"]], got["poses"], got["points"], got["objects"])
    at = dict(joint, poses=got["poses"], points=got["points"], objects=got["objects"])
    r = Reference(at, od, [(members, mean, cov)], 1e6)
    ids = np.arange(O)
    a, b = np.array([(i, j) for i in ids for j in ids]).T
    merged = g.object_covariances(a, b)
    e_merged = max(blocks.block_err(merged[x], r.obj_block(a[x], b[x])) for x in range(len(a)))
    g.covariance_compute()
    own = g.object_covariance_blocks(ids)
    e_own = max(blocks.block_err(own[i], r.obj_block(i, i)) for i in ids)
    pairs = [((OBJ, int(i)), (OBJ, int(j))) for i in ids for j in ids if i < j]            # shared x shared, shared x private, private x private
    ka, ia, kb, ib = zip(*[(x[0], x[1], y[0], y[1]) for x, y in pairs])
    assert g.covariance_on_pattern(ka, ia, kb, ib).all()
    rows = {(OBJ, int(i)): int(r.orow[i]) for i in ids}
    print("twelve objects, ten shared: merged route %.3e, own blocks %.3e (bar %.0e), cond %.2e" % (e_merged, e_own, BAR, r.cond))
    blocks.check_cross(g, pairs, rows, {k: od for k in rows}, r.Sigma, BAR, "twelve objects, ten shared")
    assert e_merged < BAR and e_own < BAR
    plain.close(); g.close()


# ---- 6. counted once, counted twice ---------------------------------------------------------------------------------------------------------------------------
def test_the_same_group_uploaded_by_two_members_counts_twice(sessions):
    job = dense_job(sessions, 7, False, 1e6, uploaders=(1, 2))
    try:
        a, b = np.array([(i, j) for i in IDS for j in IDS]).T
        merged = collective(job.handles, lambda m, h: h.object_covariances(a, b))
        e = max(blocks.block_err(c[x], job.ref.obj_block(a[x], b[x])) for c in merged for x in range(len(a)))
        once = Reference(job.ref.joint, 7, [job.prior], 1e6, times=1)
        apart = max(blocks.block_err(once.obj_block(i, i), job.ref.obj_block(i, i)) for i in IDS)
        print("members 1 and 2 upload the same group: against Sigma_ref with 2 Lambda %.3e (bar %.0e); with Lambda it would be %.3e" % (e, BAR, apart))
        assert e < BAR and apart > 1e-3
    finally:
        close_job(job.group, job.handles)


# ---- 7. the prior cut from a resident map ---------------------------------------------------------------------------------------------------------------------
def test_the_prior_cut_from_a_resident_map_is_the_host_pointer_upload(sessions):
    od = 7
    mean, cov = the_prior(sessions[0]["objects"], od, dense=True)
    runs = []
    with obvi_ba.Map.create(mean, cov, library=helpers.PRODUCT_LIB) as mp:
        for cut in (False, True):
            group, handles = open_shared_job(sessions, od)
            try:
                if cut:
                    handles[0].set_map_group_priors_from_map(mp, [list(IDS)], [list(IDS)], 2.0)
                else:
                    handles[0].set_map_group_priors([list(IDS)], [mean], [cov], 2.0)
                r, W, _ = handles[0].debug_linearize(T)
                out = collective(handles, lambda m, h: h.solve(helpers.ba_params(max_it=10)))
                runs.append((r[0], W[0], out[0], [(i.iteration, i.step_is_successful, i.cost) for i in handles[0].iterations()], handles[0].get_objects()))
            finally:
                close_job(group, handles)
    (r0, W0, s0, i0, x0), (r1, W1, s1, i1, x1) = runs
    eW, er = np.abs(W1 - W0).max() / np.abs(W0).max(), helpers.rel_err(r1, r0)
    worst = max(abs(x[2] - y[2]) / y[2] for x, y in zip(i1, i0))
    print("cut from the map against the host-pointer upload: W %.2e  r %.2e;  %d iterations, costs %.2e, objects %.2e" % (eW, er, s1.num_iterations, worst, np.abs(x1 - x0).max()))
    assert eW < 1e-12 and er < 1e-12
    assert s0.num_iterations == s1.num_iterations > 3 and [x[:2] for x in i0] == [x[:2] for x in i1] and worst <= 1e-8


# ---- 8. fold back, whole map ------------------------------------------------------------------------------------------------------------------------------------
def posterior_of(h, ids, od):
    """(means, covariance) of a member's objects `ids` through the collective obvi_ba_object_covariances and get_objects -- what the host-pointer forms are fed"""
    k = len(ids)
    c = h.object_covariances(np.repeat(ids, k), np.tile(ids, k))
    return h.get_objects()[ids], c.reshape(k, k, od, od).transpose(0, 2, 1, 3).reshape(k * od, k * od)


@pytest.fixture(scope="module")
def folded(solved):
    """every member of case 3's job conditions a map of the ten objects on all ten: (mean, cov) per member, and what each member's own posterior is"""
    with obvi_ba.Map.create(solved.mean, solved.cov, library=helpers.PRODUCT_LIB) as mp:
        before = solved.group.stats()[0]
        new = collective(solved.handles, lambda m, h: mp.condition_on(h, IDS, IDS))
        per_pass = solved.group.stats()[0] - before
        maps = [n.get() for n in new]
        for n in new:
            n.close()
        post = collective(solved.handles, lambda m, h: posterior_of(h, IDS, 7))
        fed = []
        for h, (m, P) in zip(solved.handles, post):
            with mp.condition(h, IDS, m, P) as f:
                fed.append(f.get())
    return types.SimpleNamespace(maps=maps, post=post, fed=fed, per_pass=per_pass)


def test_fold_back_the_whole_map(solved, folded):
    od = 7
    assert folded.per_pass == 4                                                          # tail order, shared blocks, tail, scalars: once per member
    want = solved.ref.obj_part(IDS)
    for m, ((mu, cv), (fmu, fcv), (pm, pP), h) in enumerate(zip(folded.maps, folded.fed, folded.post, solved.handles)):
        assert np.array_equal(mu, folded.maps[0][0]) and np.array_equal(cv, folded.maps[0][1])          # (i) deterministic members behind the compiled group
        assert np.array_equal(mu, fmu) and np.array_equal(cv, fcv)                                      # (ii) the host-pointer form fed the member's own posterior
        e = worst_block(cv, want, od)
        print("member %d: the whole map folded back against Sigma_ref's object part %.3e (bar %.0e)" % (m, e, BAR))
        assert e < BAR                                                                                  # (iii) k covers the map: the posterior itself
        assert np.array_equal(mu, h.get_objects()[IDS]) and np.array_equal(cv, cv.T)


# ---- 9. fold back, part of the map, and growth -------------------------------------------------------------------------------------------------------------------
def test_fold_back_part_of_the_map_and_growth(solved):
    od = 7
    hs = solved.handles
    part = np.array([7, 2, 9, 0, 4, 5], np.uint32)
    old, fresh = IDS[:8], IDS[8:]

    def err(got, mu_ref, C_ref):
        return max(float(np.abs(got[1] - C_ref).max() / np.abs(C_ref).max()), float(np.abs(got[0] - mu_ref).max() / np.abs(mu_ref).max()))
    with obvi_ba.Map.create(solved.mean, solved.cov, library=helpers.PRODUCT_LIB) as mp, mp.select(hs[0], old) as mp8:
        mean8, cov8 = mp8.get()
        # condition_on with six of the ten
        new = collective(hs, lambda m, h: mp.condition_on(h, part, part))
        got = [n.get() for n in new]
        [n.close() for n in new]
        post = collective(hs, lambda m, h: posterior_of(h, part, od))
        for m, (h, (pm, pP)) in enumerate(zip(hs, post)):
            with mp.condition(h, part, pm, pP) as f:
                fed = f.get()
            assert np.array_equal(got[m][0], fed[0]) and np.array_equal(got[m][1], fed[1])
            e = err(got[m], *map_update_cases.update_formula(solved.mean, solved.cov, part, pm, pP, od))
            print("member %d: six of ten objects conditioned, against numpy's update formula %.2e (bar 1e-11)" % (m, e))
            assert e <= 1e-11 and np.array_equal(got[m][0], got[0][0]) and np.array_equal(got[m][1], got[0][1])
        # extend_on: a map of eight grows by two
        new = collective(hs, lambda m, h: mp8.extend_on(h, old, old, fresh))
        got = [n.get() for n in new]
        [n.close() for n in new]
        post = collective(hs, lambda m, h: posterior_of(h, IDS, od))
        for m, (h, (pm, pP)) in enumerate(zip(hs, post)):
            with mp8.extend(h, old, pm, pP, len(fresh)) as f:
                fed = f.get()
            assert got[m][0].shape == (N_OBJ, od) and np.array_equal(got[m][0], fed[0]) and np.array_equal(got[m][1], fed[1])
            e = err(got[m], *map_extend_cases.extension_formula(mean8, cov8, old, len(fresh), pm, pP, od))
            print("member %d: a map of eight grown by two, against numpy's extension formula %.2e (bar 1e-11)" % (m, e))
            assert e <= 1e-11 and np.array_equal(got[m][1], got[0][1])
        # no map yet: a first map is born on every member
        new = collective(hs, lambda m, h: obvi_ba.Map.from_handle(h, IDS))
        got = [n.get() for n in new]
        [n.close() for n in new]
        for m, (h, (pm, pP)) in enumerate(zip(hs, post)):
            with obvi_ba.Map.from_posterior(h, pm, pP) as f:
                fed = f.get()
            assert np.array_equal(got[m][0], fed[0]) and np.array_equal(got[m][1], fed[1])
            e = err(got[m], *map_extend_cases.extension_formula(None, None, [], N_OBJ, pm, pP, od))
            assert e <= 1e-11 and np.array_equal(got[m][1], got[0][1])


# ---- 10. a member with nothing to fold -----------------------------------------------------------------------------------------------------------------------------
def test_a_member_with_nothing_to_fold_joins_through_object_covariances(solved, folded):
    with obvi_ba.Map.create(solved.mean, solved.cov, library=helpers.PRODUCT_LIB) as mp:
        before = solved.group.stats()[0]
        res = collective(solved.handles, lambda m, h: mp.condition_on(h, IDS, IDS) if m != 3 else h.object_covariances([]))
        assert solved.group.stats()[0] - before == 4 and res[3].shape[0] == 0
        for m in range(3):
            mu, cv = res[m].get()
            res[m].close()
            assert np.array_equal(mu, folded.maps[m][0]) and np.array_equal(cv, folded.maps[m][1])


# ---- 11. symmetric argument errors -------------------------------------------------------------------------------------------------------------------------------
def test_symmetric_argument_errors_enter_no_collective(sessions):
    od = 7
    mean, cov = the_prior(sessions[0]["objects"], od, dense=True)
    group, handles = open_shared_job(sessions, od)
    try:
        flags = np.zeros(N_OBJ, np.uint8); flags[4] = 1
        for h in handles:
            h.set_const_flags(object_const=flags)
        with obvi_ba.Map.create(mean, cov, library=helpers.PRODUCT_LIB) as mp:
            before = group.stats()

            def says(call, text):
                res = dist_util.run_members([lambda m=m, h=h: call(m, h) for m, h in enumerate(handles)], GROUP_TIMEOUT)
                assert all(isinstance(r, obvi_ba.ObviError) and "status -1 " + text in str(r) for r in res), res
            says(lambda m, h: mp.condition_on(h, [3, 4], [3, 4]), "map_condition_on_handle: a constant object has no posterior")
            says(lambda m, h: mp.extend_on(h, [3], [3], [4]), "map_extend_on_handle: a constant object has no posterior")
            says(lambda m, h: mp.condition_on(h, [3, 5], [6, 6]), "map_condition_on_handle: a map object twice")
            says(lambda m, h: mp.extend_on(h, [3, 5], [6, 6], [7]), "map_extend_on_handle: a map object twice")
            assert group.stats() == before                                              # no collective was entered
    finally:
        close_job(group, handles)


def test_rank_deficiency_on_one_member_fails_the_fold_on_every_member(sessions):
    """include/obvi_map_shared.h: rank-deficient normal equations on ONE member are OBVI_ERR_NUMERICAL on EVERY member, from the same call and within the group's
    time-out (the construction of test_priors_on_a_shared_object_and_symmetric_failure: member 3 floats freely); the group serves the next valid pass."""
    od = 7
    mean, cov = the_prior(sessions[0]["objects"], od, dense=True)
    group, handles = open_shared_job(sessions, od)
    try:
        q = sessions[3]
        handles[3].set_const_flags(pose_const=np.zeros(len(q["poses"]), np.uint8))
        handles[3].set_active_mask(2, np.zeros(len(q["bb_obj"]), np.uint8))
        with obvi_ba.Map.create(mean, cov, library=helpers.PRODUCT_LIB) as mp:
            assert statuses(handles, lambda m, h: mp.condition_on(h, IDS, IDS), timeout_s=GROUP_TIMEOUT + 30) == [-6] * 4
            assert statuses(handles, lambda m, h: obvi_ba.Map.from_handle(h, IDS), timeout_s=GROUP_TIMEOUT + 30) == [-6] * 4
            handles[3].set_const_flags(pose_const=q["pose_const"])
            handles[3].set_active_mask(2, np.ones(len(q["bb_obj"]), np.uint8))
            new = collective(handles, lambda m, h: mp.condition_on(h, IDS, IDS))
            assert all(n.n_objects == N_OBJ for n in new)
            [n.close() for n in new]
    finally:
        close_job(group, handles)


# ---- 12. two ranks of two handles -----------------------------------------------------------------------------------------------------------------------------------
def _fold_worker(rank, world, port, sessions, out):
    import os
    import sys
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK="0")
    sys.path.insert(0, os.path.join(helpers.ROOT, "obvi-slam_amd", "python")); sys.path.insert(0, os.path.join(helpers.ROOT, "tests"))
    import torch.distributed as dist
    dist.init_process_group(backend="gloo", rank=rank, world_size=world)
    torch.cuda.set_device(0)
    k = len(sessions) // world
    log = dist_util.IssueLog()
    group = dist_util.RcclGroup(k, inner=dist_util.staged_allreduce(dist, log), rank=rank, world=world, device=0)
    group.set_timeout(GROUP_TIMEOUT)
    handles = []
    for m in range(k):
        q = sessions[rank * k + m]
        ba = helpers.product_ba()
        synth.upload(ba, q)
        group.attach(m, ba, np.ones(len(q["objects"]), np.uint8))
        ba.map_allow_exchange(True)
        handles.append(ba)
    mean, cov = the_prior(sessions[0]["objects"], 7, dense=True)
    if rank == 1:
        handles[1].set_map_group_priors([list(IDS)], [mean], [cov], 1e6)                 # global member 3
    solve_job(handles)
    calls0 = log.calls
    with obvi_ba.Map.create(mean, cov, library=helpers.PRODUCT_LIB) as mp:
        new = collective(handles, lambda m, h: mp.condition_on(h, IDS, IDS))
        maps = [n.get() for n in new]
        [n.close() for n in new]
    per_pass = log.calls - calls0
    same = dist_util.same_issue_order(dist, log.calls, log.digest())
    out[rank] = dict(same=same, per_pass=per_pass, maps=maps)
    close_job(group, handles)
    dist.barrier()
    dist.destroy_process_group()


def test_two_ranks_of_two_handles(sessions, folded):
    import socket
    import torch.multiprocessing as mp
    sock = socket.socket(); sock.bind(("127.0.0.1", 0)); port = sock.getsockname()[1]; sock.close()
    mgr = mp.Manager(); out = mgr.dict()
    mp.spawn(_fold_worker, args=(2, port, sessions, out), nprocs=2, join=True)
    assert set(out.keys()) == {0, 1}
    want_mu, want_cv = folded.maps[0]
    for rank in (0, 1):
        o = out[rank]
        assert o["same"] and o["per_pass"] == 4                                         # one inter-rank collective per group collective, the same order on both ranks
        for m, (mu, cv) in enumerate(o["maps"]):
            e, em = worst_block(cv, want_cv, 7), float(np.abs(mu - want_mu).max())
            print("rank %d handle %d: the folded map against the one-rank job's %.3e (bar %.0e), means %.3e" % (rank, m, e, BAR, em))
            assert e < BAR and em < BAR
