"""CPU: the host format builders are deterministic -- tests/host_format_digest.cpp prints one line of FNV-1a digests per
(matrix, format) over every array the four builders produce, and the lines are the same with one builder thread and with four.
That property is what makes a comparison of the program's output between two commits (built with the same compiler and flags, run
on one machine) a complete test of a change that must leave the formats alone.  No digest value is committed: std::sort may
place equal elements differently in another standard library."""
import os
import shutil
import subprocess

import pytest

from conftest import ROOT

BUILDER_SOURCES = ("panel_format.cpp", "panel_order.cpp", "team_format.cpp", "team_cluster.cpp", "team2_format.cpp", "team2r_format.cpp",
                   "team_order.cpp", "locality.cpp", "knobs.cpp")
MATRICES = 12
# panel4, panel8, panel8.cv, teams4, team2c, team2f, team2r4, team2r2, and the device path's team2, team2r4, team2r2
LINES_PER_MATRIX = 11


def test_format_digest_is_independent_of_the_thread_count(tmp_path):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++")
    src = os.path.join(ROOT, "crp-spmm_amd", "csrc")
    exe = str(tmp_path / "host_format_digest")
    cmd = [gxx, "-std=c++17", "-O1", "-pthread", "-I" + os.path.join(ROOT, "include"), "-I" + src,
           os.path.join(ROOT, "tests", "host_format_digest.cpp"), *[os.path.join(src, f) for f in BUILDER_SOURCES], "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    outs = []
    for threads in ("1", "4"):
        env = dict(os.environ, CRPSPMM_NUM_THREADS=threads, CRPSPMM_SYNC_RELEASE="1")
        env.pop("CRPSPMM_TIMING", None)
        r = subprocess.run([exe], capture_output=True, text=True, timeout=600, env=env)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        outs.append(r.stdout.splitlines())
    assert len(outs[0]) == MATRICES * LINES_PER_MATRIX, "%d lines" % len(outs[0])
    differing = [(a, b) for a, b in zip(outs[0], outs[1]) if a != b]
    assert len(outs[0]) == len(outs[1]) and not differing, "1 thread against 4:\n%s\n%s" % differing[0]
    # every grouping of build_teams is among the matrices: lattice teams, consecutive panels, clusters (alone, and chosen over a
    # detected lattice: matrix 10 has lattice teams of four and clustered teams of eight)
    text = "\n".join(outs[0])
    assert " 0 team2c      nteam=228 lattice=1" in text and "10 teams4      nteam=456 lattice=1" in text and "10 team2c      nteam=188 lattice=0" in text
    assert " 9 team2c      nteam=600 lattice=0" in text
