"""What the library calls share around their device entries (finch_rs_amd/csrc/fh_entries.h), on its own and without a GPU:
the first-error keeper, the thread per entry, and the loop that launches m + 1 before it takes m.
tests/hostcore/entries_host.cpp includes that header and nothing else of the library, and runs one scenario per call.  Built
twice into pytest's temporary directory, plainly and under ThreadSanitizer, which must stay silent.  A deadlock shows as the
driver's timeout."""
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "hostcore", "entries_host.cpp")
INC = os.path.join(HERE, "..", "finch_rs_amd", "csrc")

SCENARIOS = {
    1: "two_slot with n = 0, 1, 2, 5: L0 [L1] T0 [L2] T1 ..., the slots alternate",
    2: "a launch fails at m + 1 = 3: take 2 is not called, the code comes back",
    3: "a take fails at m = 1: launch 2 has happened, launch 3 and take 2 have not",
    4: "another thread's fail() between iterations: 0, no further launch",
    5: "sixteen threads fail at once: one consistent (rc, msg) survives",
    6: "for_entries with n = 1, 3, 16: every entry once, bad_alloc is the capacity code, each cleanup runs once",
}


@pytest.fixture(scope="module", params=["plain", "tsan"])
def driver(request, tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("entries_" + request.param) / "entries_host")
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
