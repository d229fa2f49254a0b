"""The host rules of the clustering calls (finch_rs_amd/csrc/fh_cluster.h) on their own and without a GPU:
tests/hostcore/cluster_host.cpp includes that header and checks the union-find's smallest-index labels against a flood fill on
random graphs of up to 200 nodes, the validation of option index_cluster_margin, and the two bounds' order jlo < jhi.  Built
twice into pytest's temporary directory, plainly and under AddressSanitizer + UndefinedBehaviorSanitizer, which must stay
silent: two stand-alone programs, nothing is loaded into Python."""
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "hostcore", "cluster_host.cpp")
INC = os.path.join(HERE, "..", "finch_rs_amd", "csrc")


@pytest.mark.parametrize("build", ["plain", "asan_ubsan"])
def test_cluster_host_rules(build, tmp_path):
    exe = str(tmp_path / "cluster_host")
    flags = ["-O2"] if build == "plain" else ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-O1", "-g"]
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror"] + flags + ["-I", INC, "-o", exe, SRC])
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120)
    assert r.returncode == 0 and r.stderr == "", (build, r.returncode, r.stderr[-4000:])
    words = r.stdout.split()
    assert words[0] == "ok" and int(words[1]) == 8 * 4 * 4 and int(words[2]) == 13 * 14 * 3, r.stdout


def test_the_header_is_host_only():
    text = open(os.path.join(INC, "fh_cluster.h")).read()
    assert "hip" not in text.lower().replace("no hip", "") and "#include \"" not in text
