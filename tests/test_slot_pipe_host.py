"""The two-slot hand-off between a pump's reader thread and its pushing thread (finch_rs_amd/csrc/fh_slot_pipe.h), on its own
and without a GPU: tests/hostcore/slot_pipe_host.cpp includes that header and nothing else of the library, and runs one
scenario per call.  Built twice into pytest's temporary directory, plainly and under ThreadSanitizer, which must stay silent.
A deadlock shows as the driver's timeout."""
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "hostcore", "slot_pipe_host.cpp")
INC = os.path.join(HERE, "..", "finch_rs_amd", "csrc")

SCENARIOS = {
    1: "the job's own slot is released after use",
    2: "the previous job's slot is released (FASTQ host strip)",
    3: "several jobs per acquisition, released after the last (gzip)",
    4: "abort() while the producer waits in acquire()",
    5: "a producer that publishes nothing",
    6: "the consumer leaves by exception: producer blocked, producer publishing",
    7: "the producer's body throws",
}


@pytest.fixture(scope="module", params=["plain", "tsan"])
def driver(request, tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("slot_pipe_" + request.param) / "slot_pipe_host")
    flags = ["-O2"] if request.param == "plain" else ["-fsanitize=thread", "-O1", "-g"]
    subprocess.check_call(["g++", "-std=c++17", "-pthread", "-Wall"] + flags + ["-I", INC, "-o", exe, SRC])
    return exe, request.param


@pytest.mark.parametrize("scenario", sorted(SCENARIOS), ids=lambda s: "scenario%d" % s)
def test_scenario(driver, scenario):
    exe, flavour = driver
    r = subprocess.run([exe, str(scenario)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=60)
    assert r.returncode == 0, (SCENARIOS[scenario], flavour, r.returncode, r.stderr[-2000:])
    assert r.stdout.strip() == "ok", (SCENARIOS[scenario], r.stdout)
    assert "ThreadSanitizer" not in r.stderr, (SCENARIOS[scenario], r.stderr[-4000:])
