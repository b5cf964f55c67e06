"""GPU: the host mirror of the feature-based bounding-box front end (obvi-slam_amd/host/obvi_bounding_box_front_end.h) replays a detection stream -- 30 frames, one
camera, 2 classes, 5 physical objects -- through the device's association round, and must take the decisions, keep the pending list and the objects, and leave
the object observation factors that the Python restatement of the reference's whole addBoundingBoxObservations sequence does (tests/bbox_front_end_host_cases.py),
with the same stub hooks.  The restatement's own log is first held to contain every kind of event the sequence has, and no round in which competing scores lie
within 100 times the score bound of tests/test_gpu_bbox_frontend.py, so that the comparison can neither pass by never reaching a branch nor fail by rounding."""
import os
import subprocess

import pytest

import bbox_front_end_host_cases as host_cases
import helpers

HOST = os.path.join(helpers.ROOT, "obvi-slam_amd", "host")


@pytest.fixture(scope="module")
def restated():
    stream = host_cases.make_stream()
    return stream, host_cases.replay(stream)


def test_the_stream_reaches_every_branch_and_has_no_ties(restated):
    stream, r = restated
    assert len(stream) == 30 and len({b[0] for _, _, boxes in stream for b in boxes}) == 2 and len(host_cases.PHYSICAL) == 5
    assert r.ties == []                                                              # no exact or near tie the reference's own order would leave open
    kinds = {}
    for e in r.log:
        kinds.setdefault(e[1], []).append(e)
    assert kinds["open"]                                                             # a box that opens a pending object
    assert kinds["merge"]                                                            # a pending object with min_observations_for_local_est_ views merged into an object
    assert kinds["merge"][0][3] in r.objects
    assert kinds["new_object"] and len(r.objects) >= 3                               # a pending object with min_observations_ views becomes a new object
    assert kinds["discard"]                                                          # a pending object dropped by discard_candidate_after_num_frames_
    assert kinds["views_dropped"]                                                    # views dropped by the finite feature_validity_window_
    assert kinds["compete"] and kinds["compete"][0][0] == 10                         # two boxes of one frame with the same candidate
    frame10 = dict(r.rounds)[10]
    assert sum(1 for init, _ in frame10 if init) == 2 and (10, "open", 1) in r.log   # ... and the loser opened a pending object
    assert any(not b[5] > host_cases.PARAMS["min_conf"] for _, _, boxes in stream for b in boxes)      # the confidence filter has something to drop
    assert all(len(d) == sum(1 for b in boxes if b[5] > host_cases.PARAMS["min_conf"]) for (_, d), (_, _, boxes) in zip(r.rounds, stream))


@pytest.mark.gpu
def test_the_host_mirror_replays_the_stream_as_the_restatement_does(restated, tmp_path):
    stream, r = restated
    program, path = str(tmp_path / "bbox_front_end_replay"), str(tmp_path / "stream.txt")
    lib_dir = os.path.dirname(helpers.PRODUCT_LIB)
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-pthread", "-I" + os.path.join(helpers.ROOT, "include"), "-I" + HOST, "-o", program,
                           os.path.join(helpers.ROOT, "tests", "bbox_front_end_replay.cpp"), "-L" + lib_dir, "-lobvi_ba", "-Wl,-rpath," + lib_dir])
    host_cases.write_stream(path, stream)
    run = subprocess.run(["timeout", "-k", "5", "120", program, path], capture_output=True, text=True)
    assert run.returncode == 0, run.stderr[-2000:]
    got, want = run.stdout.splitlines(), r.lines()
    assert host_cases.same_print_out(got, want) is None
    assert sum(1 for line in got if line.startswith("round ")) == 30 and any(line.startswith("factor ") for line in got)
