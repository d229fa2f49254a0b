"""An independent model of the screen's contract (include/finch_host.h, finch_index_screen): records split with
plain Python, windows enumerated with the classification rule restated in numpy, every window hashed with oracle.hash_f on the
canonical text, multiplicities counted in a dict, each reference intersected with it and the lower median taken with sorted().
It shares no code with the product."""
import struct
from functools import lru_cache

import numpy as np

from oracle import oracle as O

BLANKS = b" \t\r\n"
_COMP = bytes.maketrans(b"ACGT", b"TGCA")

# is_base[b], and the byte a base is hashed as: ACGT, acgt and U/u (as T); every other byte breaks k-mers
IS_BASE = np.zeros(256, bool)
NORMAL = np.zeros(256, np.uint8)
for _b, _n in zip(b"ACGTUacgtu", b"ACGTTACGTT"):
    IS_BASE[_b] = True
    NORMAL[_b] = _n


def records(text: bytes):
    """the sequence() of every record of a FASTA or FASTQ text, blanks still inside"""
    if not text:
        return []
    if text[:1] == b">":
        out, cur = [], None
        for line in text.split(b"\n"):
            if line[:1] == b">":
                if cur is not None:
                    out.append(b"".join(cur))
                cur = []
            elif cur is not None:
                cur.append(line)
        if cur is not None:
            out.append(b"".join(cur))
        return out
    assert text[:1] == b"@", "neither FASTA nor FASTQ"
    lines = [ln.rstrip(b"\r") for ln in text.split(b"\n")]
    out, i = [], 0
    while i < len(lines):
        if lines[i] == b"":
            i += 1
            continue
        assert lines[i][:1] == b"@" and lines[i + 2][:1] == b"+"
        out.append(lines[i + 1])
        i += 4
    return out


def canonical_windows(seq: bytes, k: int):
    """(positions of the record, the canonical k-mer of every valid window)"""
    a = np.frombuffer(bytes(b for b in seq if b not in BLANKS), np.uint8)
    n = len(a)
    if n < k:
        return n, []
    good = IS_BASE[a].astype(np.int64)
    run = np.concatenate([[0], np.cumsum(good)])
    valid = (run[k:] - run[:n - k + 1]) == k  # every one of the k positions is a base
    norm = NORMAL[a].tobytes()
    out = []
    for p in np.nonzero(valid)[0]:
        f = norm[p:p + k]
        r = f.translate(_COMP)[::-1]
        out.append(min(f, r))
    return n, out


@lru_cache(None)
def multiplicities(texts: tuple, k: int, seed: int):
    """texts: the decompressed inputs, read as one sample -> ({hash: windows with it}, positions, valid windows)"""
    mult, positions, kmers = {}, 0, 0
    for text in texts:
        for seq in records(text):
            n, wins = canonical_windows(seq, k)
            positions += n
            kmers += len(wins)
            for w in wins:
                h = O.hash_f(w, seed)
                mult[h] = mult.get(h, 0) + 1
    return mult, positions, kmers


def screen(ref_hashes, texts, k: int, seed: int, min_shared: int = 1):
    """ref_hashes: per reference its hashes -> (rows (reference, shared, ref_len, median_mult, sum_mult, containment bits),
    stats dict)"""
    mult, positions, kmers = multiplicities(tuple(texts), k, seed)
    library = set()
    rows = []
    for r, hs in enumerate(ref_hashes):
        hs = [int(h) for h in hs]
        library.update(hs)
        ms = sorted(mult[h] for h in hs if h in mult)
        if len(ms) >= max(1, min_shared):
            rows.append((r, len(ms), len(hs), ms[(len(ms) - 1) // 2], sum(ms), struct.pack("<d", len(ms) / len(hs))))
    if not library or not any(len(t) for t in texts):
        # the contract's empty cases (include/finch_host.h): nothing is read, every figure is 0 -- and no row can exist
        assert not rows
        return rows, dict(positions=0, kmers=0, hits=0, distinct=0)
    stats = dict(positions=positions, kmers=kmers, hits=sum(m for h, m in mult.items() if h in library), distinct=len(library))
    return rows, stats


def rows_of(arr):
    """a SCREEN_DTYPE array in the model's form"""
    return [(int(x["reference"]), int(x["shared"]), int(x["ref_len"]), int(x["median_mult"]), int(x["sum_mult"]),
             struct.pack("<d", float(x["containment"]))) for x in arr]
