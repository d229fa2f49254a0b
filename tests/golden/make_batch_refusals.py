#!/usr/bin/env python3
"""Generate tests/golden/batch_refusals.json: what the four doors of the batch sketcher (fh_batch_new, fh_batch_new_wide,
fh_batch_new_large, fh_batch_new_counts; include/finch_hip.h) answer over a grid of parameters -- fh_last_error() verbatim, or
ACCEPTED where the parameters pass (a handle, or "no usable HIP device" on a machine without one: the parameter checks come
before the device check).

    python tests/golden/make_batch_refusals.py        # on the build whose answers are to be pinned, without a GPU

tests/test_batch_refusals.py holds every later build to this file.  The grid (a full product would be 10^5 cases):
  * parameters: every kind (and an unknown one) x k x size x scale without a mask, and x k x size with one, at 4 files and 1 MiB;
  * sizes: max_files x stage_bytes for parameters the door serves and for parameters it refuses (the parameters speak first);
  * fh_batch_new_counts: k x max_files x stage_bytes;
  * null params.
A case is [door, kind, k, size, scale, mask, max_files, stage_bytes], scale as text (there is a NaN among them); cases() below lists
them in a fixed order.  The file holds each distinct message once ("messages") and, per case in that order, the index of its
message ("answers").  CONSTRUCT names the dozen accepted cases that the test really constructs where there is a GPU
(max_files <= 4, 1 MiB).
"""
import ctypes as C
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

NO_DEVICE = "no usable HIP device (this library has no CPU path)"
COUNTS_MAX_STAGE = (1 << 21) * 768 - 4096  # a slot of fewer than 2^21 tiles of the two-bit form
DOORS = ("fh_batch_new", "fh_batch_new_wide", "fh_batch_new_large")
KINDS = (0, 1, 2, 7)
KS = (0, 1, 7, 8, 32, 33, 64, 65)
SIZES = (0, 1, 3000, 3001, 12288, 12289, 16384, 16385, 1 << 40)
SCALES = ("0.0", "0.001", "1.0", "1.5", "nan")
MASK = 0xFFFF
MAX_FILES = (0, 1, 4096, 4097)
STAGES = (100, 4096, 1 << 36, (1 << 36) + 1, COUNTS_MAX_STAGE, COUNTS_MAX_STAGE + 1)
# (kind, k, size, scale) a door serves, and one it refuses, for the grid of sizes
SERVED = {"fh_batch_new": (0, 21, 1000, "0.0"), "fh_batch_new_wide": (1, 33, 1000, "0.001"), "fh_batch_new_large": (0, 21, 5000, "0.0")}
REFUSED = {"fh_batch_new": (0, 33, 1000, "0.0"), "fh_batch_new_wide": (0, 21, 1000, "0.0"), "fh_batch_new_large": (0, 21, 1000, "0.0")}
# the dozen that are constructed where there is a GPU: [door, kind, k, size, scale, mask, max_files, stage]
CONSTRUCT = [
    ["fh_batch_new", 0, 1, 1, "0.0", 0, 4, 1 << 20], ["fh_batch_new", 0, 32, 3000, "0.0", 0, 4, 1 << 20],
    ["fh_batch_new", 1, 7, 0, "1.0", 0, 4, 1 << 20], ["fh_batch_new", 1, 32, 12288, "0.001", 0, 4, 1 << 20],
    ["fh_batch_new_wide", 0, 33, 3000, "0.0", 0, 4, 1 << 20], ["fh_batch_new_wide", 0, 64, 1, "0.0", 0, 4, 1 << 20],
    ["fh_batch_new_wide", 1, 64, 12288, "0.001", 0, 4, 1 << 20],
    ["fh_batch_new_large", 0, 1, 3001, "0.0", 0, 4, 1 << 20], ["fh_batch_new_large", 0, 32, 16384, "0.0", 0, 4, 1 << 20],
    ["fh_batch_new_large", 0, 7, 12288, "nan", 0, 4, 1 << 20],
    ["fh_batch_new_counts", 2, 1, 0, "0.0", 0, 4, 1 << 20], ["fh_batch_new_counts", 2, 7, 0, "0.0", 0, 4, 1 << 20],
]


def cases():
    """the grid, in a fixed order, as [door, kind, k, size, scale, mask, max_files, stage]; kind None = null params"""
    out = []
    for door in DOORS:
        out.append([door, None, 0, 0, "0.0", 0, 4, 1 << 20])
        for kind in KINDS:
            for k in KS:
                for size in SIZES:
                    for scale in SCALES:
                        out.append([door, kind, k, size, scale, 0, 4, 1 << 20])
                    out.append([door, kind, k, size, "0.001", MASK, 4, 1 << 20])
        for kind, k, size, scale in (SERVED[door], REFUSED[door]):
            for mf in MAX_FILES:
                for stage in STAGES:
                    out.append([door, kind, k, size, scale, 0, mf, stage])
    for k in KS:
        out.append(["fh_batch_new_counts", 2, k, 0, "0.0", 0, 4, 1 << 20])
        for mf in MAX_FILES:
            for stage in STAGES:
                out.append(["fh_batch_new_counts", 2, k, 0, "0.0", 0, mf, stage])
    seen, uniq = set(), []
    for c in out + CONSTRUCT:
        if tuple(c) not in seen:
            seen.add(tuple(c))
            uniq.append(c)
    return uniq


def ask(L, case):
    """(handle or None, message) of one door for one case; the caller frees the handle"""
    from finch_rs_amd._lib import FhParams
    door, kind, k, size, scale, mask, mf, stage = case
    if door == "fh_batch_new_counts":
        h = L.fh_batch_new_counts(k, 0, mf, stage)
    elif kind is None:
        h = getattr(L, door)(None, 0, mf, stage)
    else:
        p = FhParams(kind, k, size, 0, float(scale), 0, mask, 0)
        h = getattr(L, door)(C.byref(p), 0, mf, stage)
    return h, ("" if h else (L.fh_last_error() or b"").decode(errors="replace"))


def main():
    from finch_rs_amd import _lib
    L = _lib.load()
    if L.fh_device_count() > 0:
        sys.exit("run this without a GPU: the accepted cases of the grid would each construct a handle")
    messages, index, answers = [], {}, []
    for case in cases():
        h, msg = ask(L, case)
        assert not h
        msg = "ACCEPTED" if msg == NO_DEVICE else msg
        if msg not in index:
            index[msg] = len(messages)
            messages.append(msg)
        answers.append(index[msg])
        assert case not in CONSTRUCT or msg == "ACCEPTED", case
    with open(os.path.join(HERE, "batch_refusals.json"), "w") as f:
        f.write('{"_generator": "tests/golden/make_batch_refusals.py",\n "messages": %s,\n "answers": [\n' % json.dumps(messages, indent=1))
        f.write(",\n".join(", ".join(str(a) for a in answers[i:i + 60]) for i in range(0, len(answers), 60)))
        f.write("\n]}\n")
    print("%d cases, %d messages, %d accepted" % (len(answers), len(messages), sum(messages[a] == "ACCEPTED" for a in answers)))


if __name__ == "__main__":
    main()
