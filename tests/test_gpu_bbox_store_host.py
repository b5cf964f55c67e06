"""GPU: the host mirror of the feature-based bounding-box front end in store mode (obvi-slam_amd/host/obvi_bounding_box_front_end.h, useAppearanceStore) replays the
detection stream of tests/test_gpu_bbox_front_end_host.py and must print what the Python restatement of the reference's sequence prints
(tests/bbox_front_end_host_cases.py): the same decisions, events (open, merge, new_object, discard, views_dropped, compete), pending list, objects, view sizes and
factors as the host path.  The store starts with a pool of 32 ids and compacts from one dead id on, so the stream grows and compacts it."""
import os
import subprocess

import pytest

import bbox_front_end_host_cases as host_cases
import helpers

HOST = os.path.join(helpers.ROOT, "obvi-slam_amd", "host")


@pytest.mark.gpu
def test_the_host_mirror_in_store_mode_replays_the_stream_as_the_restatement_does(tmp_path):
    stream = host_cases.make_stream()
    r = host_cases.replay(stream)
    program, path = str(tmp_path / "bbox_store_replay"), str(tmp_path / "stream.txt")
    lib_dir = os.path.dirname(helpers.PRODUCT_LIB)
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-pthread", "-I" + os.path.join(helpers.ROOT, "include"), "-I" + HOST, "-o", program,
                           os.path.join(helpers.ROOT, "tests", "bbox_store_replay.cpp"), "-L" + lib_dir, "-lobvi_ba", "-Wl,-rpath," + lib_dir])
    host_cases.write_stream(path, stream)
    run = subprocess.run(["timeout", "-k", "5", "120", program, path], capture_output=True, text=True)
    assert run.returncode == 0, run.stderr[-2000:]
    got, want = run.stdout.splitlines(), r.lines()
    assert got[-1].startswith("store owners ")
    words = got[-1].split()
    stats = dict(zip(words[1::2], (int(w) for w in words[2::2])))
    print(got[-1])
    assert host_cases.same_print_out(got[:-1], want) is None
    assert sum(1 for line in got if line.startswith("round ")) == 30 and any(line.startswith("factor ") for line in got)
    assert any(line.startswith("event ") and " views_dropped " in line for line in got) and any(" merge " in line for line in got)
    assert stats["compactions"] >= 1 and stats["growths"] >= 1
    assert stats["owners"] == len(r.pending) + len(r.appearance)
