"""The streamed rule of k_record_stream (finch_rs_amd/csrc/fh_records.hip), stated in Python over a record's windows in record
order: a window whose hash is above the threshold T is dropped at once; the others wait until a fold, which merges them into the
running list L (distinct hashes ascending, counts added), cuts L (Mash: the first `size`; Scaled: every hash at or below
max_hash and the first `size` whatever their hash) and lowers T (Mash: L[size - 1] once L has `size` entries; Scaled: never
below max_hash).  Nothing here knows how the kernel sorts or where it keeps things: the model pins the exactness argument -- a
dropped window is in no final sketch, a hash of the final sketch was never dropped and so carries all its occurrences."""
import bisect

U64_MAX = (1 << 64) - 1
MASH, SCALED = 0, 1


def windows_of(record: bytes, k: int, seed: int, hash_f, reverse_complement):
    """[(hash, canonical k-mer, is_rc)] of the valid windows of `record` (upper-case bases; any other byte breaks a window), in
    record order; the canonical k-mer is the smaller of the window and its reverse complement, the reverse complement on a tie"""
    out = []
    for i in range(len(record) - k + 1):
        w = record[i:i + k]
        if w.strip(b"ACGT"):
            continue
        rc = reverse_complement(w)
        canon, is_rc = (w, 0) if w < rc else (rc, 1)
        out.append((hash_f(canon, seed), canon, is_rc))
    return out


def streamed_sketch(windows, kind: int, size: int, max_hash: int, fold_every: int, cap=None):
    """-> ([(hash, k-mer, count, extra_count)] ascending, folds, dropped), or None if a list outgrows `cap` (the kernel's "not taken")"""
    state = {"T": U64_MAX, "folds": 0}
    entry, heads = {}, []  # L: hash -> [k-mer, count, extra_count], and its hashes ascending
    pending = []

    def fold():
        for h, km, is_rc in pending:
            if h in entry:
                assert entry[h][0] == km, "a 64-bit collision"
                entry[h][1] += 1
                entry[h][2] += is_rc
            else:
                entry[h] = [km, 1, is_rc]
                bisect.insort(heads, h)
        del pending[:]
        # kept: rank < size, or (Scaled) hash <= max_hash -- both monotone in the rank, so a prefix of the heads
        n_keep = max(min(size, len(heads)), bisect.bisect_right(heads, max_hash) if kind == SCALED else 0)
        if cap is not None and n_keep > cap:
            return False
        for h in heads[n_keep:]:
            del entry[h]
        del heads[n_keep:]
        t_size = U64_MAX if len(heads) < size else (heads[size - 1] if size else 0)
        state["T"] = max(max_hash, t_size) if kind == SCALED else t_size
        state["folds"] += 1
        return True

    dropped = 0
    for i, (h, km, is_rc) in enumerate(windows):
        if h <= state["T"]:  # (one EQUAL to T is an occurrence to count)
            pending.append((h, km, is_rc))
        else:
            dropped += 1
        if (i + 1) % fold_every == 0 and not fold():
            return None
    if not fold():
        return None
    return [(h, entry[h][0], entry[h][1], entry[h][2]) for h in heads], state["folds"], dropped
