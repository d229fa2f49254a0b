"""A DEFLATE (RFC 1951) encoder for tests -- not a compressor.  Every stream the other inflate tests feed the decoders
comes out of zlib, and zlib writes a subset of the format: no distance above 32 506, no code chosen for its length, no
header shape but its own.  This module turns a list of blocks -- type, final flag, tokens (a literal byte or a
(length, distance) pair), and for a dynamic block its two code-length vectors and the way its header is written -- into
raw DEFLATE bytes, wraps them in gzip / BGZF containers, and holds the corpus the shape tests share:

  corpus().accepted   streams zlib inflates (test_deflate_writer.py says so), one per shape the decoders have seams at
  corpus().refused    streams zlib refuses: a short valid prefix, then one fault each

Plain Python + numpy; the census in test_deflate_writer.py reads the `stats` every written block leaves behind."""
import bisect
import functools
import math
import struct
import zlib

import numpy as np

LEN_BASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
LEN_EXTRA = [0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0]
DIST_BASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145,
             8193, 12289, 16385, 24577]
DIST_EXTRA = [0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13]
CL_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]
FIXED_LL = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8
FIXED_DL = [5] * 32
EOB = 256


def length_symbol(length, as_284=False):
    """(symbol, extra bits, extra value); 258 has two spellings: symbol 285, or 284 with all five extra bits set"""
    if length == 258:
        return (284, 5, 31) if as_284 else (285, 0, 0)
    i = bisect.bisect_right(LEN_BASE, length) - 1
    return 257 + i, LEN_EXTRA[i], length - LEN_BASE[i]


def distance_symbol(dist):
    i = bisect.bisect_right(DIST_BASE, dist) - 1
    return i, DIST_EXTRA[i], dist - DIST_BASE[i]


class BitWriter:
    """LSB-first: the first bit written is bit 0 of the first byte"""

    def __init__(self):
        self.out = bytearray()
        self.acc = 0
        self.n = 0

    def bits(self, value, nbits):
        self.acc |= (value & ((1 << nbits) - 1)) << self.n
        self.n += nbits
        while self.n >= 32:
            self.out += (self.acc & 0xFFFFFFFF).to_bytes(4, "little")
            self.acc >>= 32
            self.n -= 32

    def bitpos(self):
        return len(self.out) * 8 + self.n

    def align(self):
        if self.n & 7:
            self.bits(0, 8 - (self.n & 7))

    def raw(self, data):
        assert self.n % 8 == 0
        self.out += self.acc.to_bytes(self.n // 8, "little") + bytes(data)
        self.acc = self.n = 0

    def getvalue(self):
        self.align()
        return bytes(self.out) + self.acc.to_bytes(self.n // 8, "little")


def _reverse(code, nbits):
    r = 0
    for _ in range(nbits):
        r = (r << 1) | (code & 1)
        code >>= 1
    return r


def canonical_codes(lengths):
    """RFC 1951 3.2.2; the codes come back bit-reversed, ready for an LSB-first writer.  An over-subscribed set still gets
    codes (cut to their lengths): such a header is refused before any of them is looked at."""
    count = [0] * 16
    for l in lengths:
        count[l] += 1
    count[0] = 0
    nxt, code = [0] * 16, 0
    for l in range(1, 16):
        code = (code + count[l - 1]) << 1
        nxt[l] = code
    codes = [0] * len(lengths)
    for s, l in enumerate(lengths):
        if l:
            codes[s] = _reverse(nxt[l] & ((1 << l) - 1), l)
            nxt[l] += 1
    return codes


def fit_lengths(freqs, maxbits=15, force=None):
    """Code lengths <= maxbits for the symbols with a frequency, COMPLETE whatever `force` ({symbol: length}) pins down: the
    forced symbols take their share of the code space, the others are dealt the rest in order of frequency, each the length
    nearest its Shannon length that still lets the symbols behind it fill what is left exactly (space S can be filled by m
    codes iff popcount(S) <= m <= S, in units of 2^-maxbits).  Near-Huffman for a natural histogram, and any length class
    can be reached on request.  One symbol alone gets length 1 (the incomplete code DEFLATE allows)."""
    n = len(freqs)
    force = dict(force or {})
    lens = [0] * n
    unit = 1 << maxbits
    space = unit
    for s, l in force.items():
        lens[s] = l
        space -= unit >> l
    rest = sorted((s for s in range(n) if freqs[s] > 0 and s not in force), key=lambda s: (-freqs[s], s))
    m = len(rest)
    if m == 0:
        return lens
    if m == 1 and space == unit:
        lens[rest[0]] = 1
        return lens
    assert bin(space).count("1") <= m <= space, "the forced lengths leave no room for a complete code"
    total = float(sum(freqs[s] for s in rest))
    share = space / unit
    for idx, s in enumerate(rest):
        left = m - idx - 1
        ideal = -math.log2(freqs[s] / total * share)
        for l in sorted(range(1, maxbits + 1), key=lambda l: (abs(l - ideal), l)):
            s2 = space - (unit >> l)
            if s2 < 0:
                continue
            if (s2 == 0) if left == 0 else (bin(s2).count("1") <= left <= s2):
                break
        else:
            raise AssertionError("no complete code")
        lens[s] = l
        space = s2
    assert space == 0
    return lens


def rle_lengths(parts, runs=True):
    """the code-length sequence(s) as symbols of the code-length alphabet: [(symbol, extra value)].  A run never crosses from
    one part into the next; hand the literal/length and distance lengths over as ONE part to let runs cross HLIT."""
    out = []
    for seq in parts:
        i = 0
        while i < len(seq):
            v = seq[i]
            j = i
            while j < len(seq) and seq[j] == v:
                j += 1
            r = j - i
            i = j
            if not runs:
                out += [(v, 0)] * r
                continue
            if v == 0:
                while r >= 11:
                    k = min(r, 138)
                    out.append((18, k - 11))
                    r -= k
                if r >= 3:
                    out.append((17, r - 3))
                    r = 0
                out += [(0, 0)] * r
            else:
                out.append((v, 0))
                r -= 1
                while r >= 3:
                    k = min(r, 6)
                    out.append((16, k - 3))
                    r -= k
                out += [(v, 0)] * r
    return out


CL_EXTRA = {16: 2, 17: 3, 18: 7}


class Block:
    """kind: 'stored' (data), 'fixed' or 'dynamic' (tokens).  Tokens: an int (literal), (length, distance), ('L', symbol) -- a
    raw literal/length symbol without extra bits -- or ('M', length, distance symbol, extra value) -- a match through a raw
    distance symbol; the last two exist for the refused streams.  Header options of a dynamic block (all optional):
      ll, dl          the code-length vectors (default: fit_lengths of the block's histogram, with ll_force / dl_force)
      hlit, hdist     lengths sent (default: up to the last non-zero one; at least 257 / 1)
      hclen           code-length-code lengths sent (default: as few as possible)
      runs, cross     use symbols 16 / 17 / 18; may a run cross from the literal/length lengths into the distance lengths
      cl_lens, cl_force, cl_syms   the code-length code itself / forced lengths in it / the symbol sequence itself
      hlit_field, hdist_field, btype, nlen, eob   raw header fields, a wrong NLEN, no end-of-block (refused streams)
      as_284          spell length 258 as symbol 284 + 31"""

    def __init__(self, kind, tokens=(), data=b"", final=False, **opts):
        self.kind, self.tokens, self.data, self.final, self.opts = kind, list(tokens), bytes(data), final, opts
        self.stats = None


def _histogram(tokens, as_284):
    lf, df = [0] * 286, [0] * 30
    lf[EOB] = 1
    for t in tokens:
        if isinstance(t, int):
            lf[t] += 1
        elif t[0] == "L":
            pass
        elif t[0] == "M":
            lf[length_symbol(t[1], as_284)[0]] += 1
        else:
            lf[length_symbol(t[0], as_284)[0]] += 1
            df[distance_symbol(t[1])[0]] += 1
    return lf, df


def write_block(bw, blk):
    """appends the block; blk.stats: what a census wants to know about it"""
    o = blk.opts
    st = blk.stats = dict(kind=blk.kind, start_bit=bw.bitpos(), n_tokens=len(blk.tokens))
    btype = o.get("btype", {"stored": 0, "fixed": 1, "dynamic": 2}[blk.kind])
    bw.bits(1 if blk.final else 0, 1)
    bw.bits(btype, 2)
    if blk.kind == "stored":
        bw.align()
        bw.bits(len(blk.data), 16)
        bw.bits(o.get("nlen", len(blk.data) ^ 0xFFFF), 16)
        bw.raw(blk.data)
        st["end_bit"] = bw.bitpos()
        return
    as_284 = o.get("as_284", False)
    if blk.kind == "fixed":
        ll, dl = FIXED_LL, FIXED_DL
    else:
        lf, df = _histogram(blk.tokens, as_284)
        ll = list(o["ll"]) if "ll" in o else fit_lengths(lf, 15, o.get("ll_force"))
        dl = list(o["dl"]) if "dl" in o else fit_lengths(df, 15, o.get("dl_force"))
        hlit = o.get("hlit") or max(257, max((i + 1 for i, l in enumerate(ll) if l), default=0))
        hdist = o.get("hdist") or max(1, max((i + 1 for i, l in enumerate(dl) if l), default=0))
        ll = (ll + [0] * 288)[:hlit]
        dl = (dl + [0] * 32)[:hdist]
        parts = [ll + dl] if o.get("cross", True) else [ll, dl]
        syms = o["cl_syms"] if "cl_syms" in o else rle_lengths(parts, o.get("runs", True))
        if "cl_lens" in o:
            cl = list(o["cl_lens"])
        else:
            cf = [0] * 19
            for s, _ in syms:
                cf[s] += 1
            cl = fit_lengths(cf, 7, o.get("cl_force"))
            if sum(1 for l in cl if l) == 1:  # one symbol alone: the code-length code may not be incomplete
                cl[0 if cl[0] == 0 else 1] = 1
        need = max([4] + [i + 1 for i, s in enumerate(CL_ORDER) if cl[s]])
        hclen = o.get("hclen") or need
        bw.bits(o.get("hlit_field", hlit - 257), 5)
        bw.bits(o.get("hdist_field", hdist - 1), 5)
        bw.bits(hclen - 4, 4)
        for s in CL_ORDER[:hclen]:
            bw.bits(cl[s], 3)
        cc = canonical_codes(cl)
        for s, extra in syms:
            bw.bits(cc[s], cl[s])
            if s >= 16:
                bw.bits(extra, CL_EXTRA[s])
        st.update(hlit=hlit, hdist=hdist, hclen=hclen, cl_syms=list(syms), cl_lens=cl, ll=ll, dl=dl)
    lc, dc = canonical_codes(ll), canonical_codes(dl)
    ll_used, dl_used = {}, {}  # (kind, code length) -> symbols decoded through it
    pairs = dict(lit_lit={}, lit_len=0, lit_eob=0)
    prev_lit = 0  # code length of the literal just written, 0: none
    bits = bw.bits
    for t in blk.tokens:
        if isinstance(t, int):
            l = ll[t]
            bits(lc[t], l)
            ll_used[("lit", l)] = ll_used.get(("lit", l), 0) + 1
            if prev_lit:
                pairs["lit_lit"][prev_lit + l] = pairs["lit_lit"].get(prev_lit + l, 0) + 1
            prev_lit = l
            continue
        if t[0] == "L":
            bits(lc[t[1]], ll[t[1]])
            prev_lit = 0
            continue
        if t[0] == "M":
            length, (ds, de, dv) = t[1], (t[2], (DIST_EXTRA + [13, 13])[t[2]], t[3])
        else:
            length, (ds, de, dv) = t[0], distance_symbol(t[1])
        s, e, v = length_symbol(length, as_284)
        bits(lc[s], ll[s])
        bits(v, e)
        bits(dc[ds], dl[ds])
        bits(dv, de)
        ll_used[("len", ll[s])] = ll_used.get(("len", ll[s]), 0) + 1
        dl_used[dl[ds]] = dl_used.get(dl[ds], 0) + 1
        if prev_lit and prev_lit + ll[s] <= 10:
            pairs["lit_len"] += 1
        prev_lit = 0
    if o.get("eob", True):
        bits(lc[EOB], ll[EOB])
        if prev_lit and prev_lit + ll[EOB] <= 10:
            pairs["lit_eob"] += 1
    st.update(end_bit=bw.bitpos(), ll_used=ll_used, dl_used=dl_used, pairs=pairs, eob_len=ll[EOB])


def write_stream(blocks):
    bw = BitWriter()
    for b in blocks:
        write_block(bw, b)
    return bw.getvalue()


def tokens_text(blocks):
    """what the blocks spell (the model a stream's text is checked against before zlib is asked)"""
    out = bytearray()
    for b in blocks:
        if b.kind == "stored":
            out += b.data
            continue
        for t in b.tokens:
            if isinstance(t, int):
                out.append(t)
            else:
                n, d = t
                if d >= n:
                    out += out[len(out) - d:len(out) - d + n]
                else:
                    for _ in range(n):
                        out.append(out[-d])
    return bytes(out)


# ---------------------------------------------------------------------------------------------------------------------
# containers
# ---------------------------------------------------------------------------------------------------------------------
def gzip_container(raw, text, fextra=None, fname=None, fcomment=None, fhcrc=False):
    flg = (4 if fextra is not None else 0) | (8 if fname is not None else 0) | (16 if fcomment is not None else 0) | (2 if fhcrc else 0)
    h = b"\x1f\x8b\x08" + bytes([flg]) + b"\0\0\0\0\x00\xff"
    if fextra is not None:
        h += struct.pack("<H", len(fextra)) + fextra
    if fname is not None:
        h += fname + b"\0"
    if fcomment is not None:
        h += fcomment + b"\0"
    if fhcrc:
        h += struct.pack("<H", zlib.crc32(h) & 0xFFFF)
    return h + raw + struct.pack("<II", zlib.crc32(text) & 0xFFFFFFFF, len(text) & 0xFFFFFFFF)


def bgzf_member(raw, text):
    """the layout of bgzf_file in test_gpu_bgzf_device.py"""
    assert len(raw) + 25 <= 0xFFFF and len(text) <= 65536
    return (b"\x1f\x8b\x08\x04\0\0\0\0\x00\xff" + struct.pack("<H", 6) + b"BC" + struct.pack("<HH", 2, len(raw) + 25) + raw +
            struct.pack("<II", zlib.crc32(text) & 0xFFFFFFFF, len(text)))


BGZF_EOF = bgzf_member(b"\x03\x00", b"")


def bgzf_image(members, eof_marker=True):
    """members: [(raw DEFLATE bytes, their text)]"""
    return b"".join(bgzf_member(r, t) for r, t in members) + (BGZF_EOF if eof_marker else b"")


# ---------------------------------------------------------------------------------------------------------------------
# texts and tokens
# ---------------------------------------------------------------------------------------------------------------------
def fastq_text(n_reads, seed, rl_lo=30, rl_hi=300, noisy_quals=True, genome=50_000):
    """as fastq_text of the device inflate tests builds its reads, the genome drawn here (numpy alone)"""
    rng = np.random.default_rng(seed)
    g = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, size=genome)]
    recs = []
    for i in range(n_reads):
        rl = int(rng.integers(rl_lo, rl_hi + 1))
        st = int(rng.integers(0, len(g) - rl))
        seq = bytearray(g[st:st + rl].tobytes())
        if rng.random() < 0.2:
            seq[int(rng.integers(0, rl))] = ord("N")
        q = bytes(rng.integers(35, 74, size=rl, dtype=np.uint8)) if noisy_quals else b"I" * rl
        recs.append(b"@read%d/%d\n%s\n+\n%s\n" % (i, seed, bytes(seq), q))
    return b"".join(recs)


def fastq_exact(n_bytes, seed, **kw):
    """FASTQ text of exactly n_bytes: whole records, the header of the last one padded"""
    recs = fastq_text(max(8, n_bytes // 60), seed, **kw).split(b"\n")
    out, i = b"", 0
    while True:
        rec = b"\n".join(recs[4 * i:4 * i + 4]) + b"\n"
        if len(out) + len(rec) + 400 > n_bytes:
            break
        out += rec
        i += 1
    room = n_bytes - len(out)  # 60 .. 700 bytes: one padded record
    rl = min(40, (room - 12) // 2)
    pad = room - (2 * rl + 9)
    rng = np.random.default_rng(seed + 1)
    seq = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, size=rl)].tobytes()
    out += b"@pad" + b"x" * pad + b"\n" + seq + b"\n+\n" + b"I" * rl + b"\n"
    assert len(out) == n_bytes
    return out


def _common(text, a, b, limit):
    """length of the common prefix of text[a:] and text[b:], at most limit"""
    limit = min(limit, len(text) - b)
    lo, hi = 0, limit
    if text[a:a + hi] == text[b:b + hi]:
        return hi
    while hi - lo > 1:  # text[a:a+lo] matches, text[a:a+hi] does not
        mid = (lo + hi) // 2
        if text[a + lo:a + mid] == text[b + lo:b + mid]:
            lo = mid
        else:
            hi = mid
    return lo


class Stream:
    """Text and tokens grown together.  lit() / match() spell tokens out; feed() runs a small tokenizer (a hash of three bytes
    with candidate lists) over new text under a policy:
      nearest   the longest match, the nearer of equals          farthest   the largest distance <= max_dist
      chain     a source inside the previous token's output, else nearest          none   literals only
    with max_len as the 'short' policy's cap and min_len as the shortest match taken.  end_block() closes a block."""

    def __init__(self):
        self.text = bytearray()
        self.blocks = []
        self.cur = []
        self.table = {}
        self.hashed = 0

    def _index(self, upto):
        t, tab = self.text, self.table
        for i in range(self.hashed, min(upto, len(t) - 2)):
            tab.setdefault(bytes(t[i:i + 3]), []).append(i)
        self.hashed = max(self.hashed, min(upto, len(t) - 2))

    def lit(self, data):
        self.cur += list(data)
        self.text += data

    def match(self, length, dist):
        assert 3 <= length <= 258 and 1 <= dist <= 32768 and dist <= len(self.text)
        self.cur.append((length, dist))
        for _ in range(length):
            self.text.append(self.text[-dist])

    def feed(self, data, policy="nearest", max_len=258, min_len=3, max_dist=32768, max_cand=24):
        start = len(self.text)
        self.text += data
        text = bytes(self.text)
        end = len(text)
        i = start
        prev_start = start
        while i < end:
            best = None
            if policy != "none" and i + 3 <= end:
                self._index(i)
                cands = self.table.get(text[i:i + 3], ())
                lo = bisect.bisect_left(cands, i - max_dist)
                live = cands[lo:]
                if policy == "farthest":
                    for p in live[:max_cand]:
                        n = _common(text, p, i, min(max_len, end - i))
                        if n >= min_len:
                            best = (n, i - p)
                            break
                else:
                    pool = live[-max_cand:]
                    if policy == "chain":
                        inside = [p for p in pool if p >= prev_start]
                        pool = inside or pool
                    for p in reversed(pool):
                        n = _common(text, p, i, min(max_len, end - i))
                        if n >= min_len and (best is None or n > best[0]):
                            best = (n, i - p)
            prev_start = i
            if best:
                self.cur.append(best)
                i += best[0]
            else:
                self.cur.append(text[i])
                i += 1

    def end_block(self, kind="dynamic", final=False, **opts):
        self.blocks.append(Block(kind, self.cur, final=final, **opts))
        self.cur = []

    def stored(self, data, final=False, **opts):
        assert not self.cur
        self.text += data
        self.blocks.append(Block("stored", data=data, final=final, **opts))

    def cut_blocks(self, n_tokens, kind="dynamic", **opts):
        """the tokens at hand as blocks of n_tokens"""
        toks, self.cur = self.cur, []
        for i in range(0, len(toks), n_tokens):
            self.blocks.append(Block(kind, toks[i:i + n_tokens], **opts))

    def finish(self):
        if self.cur or not self.blocks:
            self.end_block()
        self.blocks[-1].final = True
        raw = write_stream(self.blocks)
        return raw, bytes(self.text)


# ---------------------------------------------------------------------------------------------------------------------
# a token reader (what did another encoder write?)
# ---------------------------------------------------------------------------------------------------------------------
def read_tokens(raw):
    """the (length, distance) pairs and the literal count of a raw DEFLATE stream, bit by bit"""
    pos = 0

    def take(n):
        nonlocal pos
        v = 0
        for k in range(n):
            v |= ((raw[(pos + k) >> 3] >> ((pos + k) & 7)) & 1) << k
        pos += n
        return v

    def decoder(lengths):
        nxt, count, code = [0] * 16, [0] * 16, 0
        for l in lengths:
            count[l] += 1
        count[0] = 0
        for l in range(1, 16):
            code = (code + count[l - 1]) << 1
            nxt[l] = code
        table = {}
        for s, l in enumerate(lengths):
            if l:
                table[(l, nxt[l])] = s
                nxt[l] += 1

        def sym():
            code = 0
            for l in range(1, 16):
                code = (code << 1) | take(1)
                if (l, code) in table:
                    return table[(l, code)]
            raise ValueError("no such code")
        return sym

    matches, n_lit = [], 0
    while True:
        final, btype = take(1), take(2)
        if btype == 0:
            pos = (pos + 7) & ~7
            n = take(16)
            take(16)
            pos += 8 * n
            n_lit += n
        else:
            if btype == 1:
                ll, dl = FIXED_LL, FIXED_DL
            else:
                hlit, hdist, hclen = take(5) + 257, take(5) + 1, take(4) + 4
                cl = [0] * 19
                for s in CL_ORDER[:hclen]:
                    cl[s] = take(3)
                cls, lens = decoder(cl), []
                while len(lens) < hlit + hdist:
                    s = cls()
                    if s < 16:
                        lens.append(s)
                    elif s == 16:
                        lens += [lens[-1]] * (3 + take(2))
                    else:
                        lens += [0] * (3 + take(3) if s == 17 else 11 + take(7))
                ll, dl = lens[:hlit], lens[hlit:]
            lsym, dsym = decoder(ll), decoder(dl)
            while True:
                s = lsym()
                if s < 256:
                    n_lit += 1
                elif s == 256:
                    break
                else:
                    n = LEN_BASE[s - 257] + take(LEN_EXTRA[s - 257])
                    d = dsym()
                    matches.append((n, DIST_BASE[d] + take(DIST_EXTRA[d])))
        if final:
            return matches, n_lit


# ---------------------------------------------------------------------------------------------------------------------
# the corpus
# ---------------------------------------------------------------------------------------------------------------------
class Case:
    """bgzf: fits one BGZF member; fastq: its text alone is a FASTQ file (the members of A7m are so only together, in the order
    1 byte, 0 bytes, 65 536 bytes)"""

    def __init__(self, cid, raw, text, blocks, bgzf=True, fastq=True):
        self.id, self.raw, self.text, self.blocks, self.bgzf, self.fastq = cid, raw, text, blocks, bgzf, fastq

    def tokens(self):
        return [t for b in self.blocks for t in b.tokens]


def _case(cid, stream, **kw):
    raw, text = stream.finish()
    assert tokens_text(stream.blocks) == text
    return Case(cid, raw, text, stream.blocks, **kw)


P = 32768


def record_cuts(text, n):
    """n + 1 offsets into FASTQ text, from 0 to its end, each at the start of a record"""
    starts, off = [], 0
    for j, ln in enumerate(text.split(b"\n")[:-1]):
        if j % 4 == 0:
            starts.append(off)
        off += len(ln) + 1
    return [starts[len(starts) * i // n] for i in range(n)] + [len(text)]


def a1_far_distances():
    """one BGZF member's worth: a period of 32 768 bytes, its first 12 KiB again (distance exactly 32 768: lengths 258, then 3),
    fresh text under the farthest policy capped at 32 767 (the 261 distances zlib never writes), and a record whose bases are
    those of a record 32 600 bytes back (length 258 at such a distance)"""
    s = Stream()
    p0 = fastq_exact(P, 41)
    s.feed(p0, "nearest")
    s.end_block()
    cuts = record_cuts(p0, 16)
    s.feed(p0[:cuts[3]], "farthest")
    s.feed(p0[cuts[3]:cuts[6]], "farthest", max_len=3)
    s.end_block()
    # a record of p0 whose sequence line is >= 262 bases, and where its copy will stand
    lines = p0.split(b"\n")
    off, src = 0, None
    for j, ln in enumerate(lines):
        if j % 4 == 1 and len(ln) >= 262 and len(s.text) - P + 700 < off < 32000:
            src = (off, ln)
        off += len(ln) + 1
    q, bases = src
    at = q + 32600  # where the copy's sequence line begins
    filler = fastq_exact(at - len(s.text) - 9, 43, noisy_quals=False)
    s.feed(filler, "farthest", max_dist=P - 1)
    s.end_block()
    s.feed(b"@copy/43\n", "none")
    assert len(s.text) == at
    s.feed(bases, "farthest", max_dist=P - 1, min_len=258)
    s.feed(b"\n+\n" + b"I" * len(bases) + b"\n", "farthest", max_dist=P - 1)
    assert len(s.text) <= 65536
    return _case("A1", s)


def a2_long_codes():
    """blocks whose literal/length code has literals, length symbols and the end-of-block code at 11..15 bits, whose distance
    code has symbols at 9..15 bits and whose code-length code has 7-bit codes"""
    s = Stream()
    text = fastq_text(110, 52)
    s.feed(text, "nearest", max_cand=4)
    toks, s.cur = s.cur, []
    per = (len(toks) + 4) // 5
    for b in range(5):
        part = toks[b * per:(b + 1) * per]
        lf, df = _histogram(part, False)
        lits = sorted((x for x in range(35, 74) if lf[x]), key=lambda x: -lf[x])[8:13]  # five quality values, not the rarest
        lsyms = sorted((x for x in range(257, 286) if lf[x]), key=lambda x: -lf[x])[:5]
        dsyms = sorted((x for x in range(30) if df[x]), key=lambda x: -df[x])[:7]
        force = {EOB: 11 + b}
        for i, x in enumerate(lits):
            force[x] = 11 + (i + b) % 5
        for i, x in enumerate(lsyms):
            force[x] = 11 + (i + b) % 5
        s.blocks.append(Block("dynamic", part, ll_force=force, dl_force={x: 9 + (i + b) % 7 for i, x in enumerate(dsyms)},
                              cl_force={0: 7, 18: 7}))
    return _case("A2", s)


def a3_258_as_284():
    s = Stream()
    s.feed(fastq_text(95, 53, rl_lo=270, rl_hi=300, noisy_quals=False), "nearest")
    s.cut_blocks(900, as_284=True)
    return _case("A3", s)


def _rec(s, name, seq_fn, qual_fn):
    s.lit(b"@" + name + b"\n")
    seq_fn()
    s.lit(b"\n+\n")
    qual_fn()
    s.lit(b"\n")


def a5_copy_match_seams(part):
    """spelled out token by token: every distance 1..9 with lengths 3..20 and 258 (the replayed pattern), distances 8..63 with a
    length above the distance (overlapping words), distance >= length with lengths 63..66, 127..130, 258 (tails of 1..7 bytes)"""
    s = Stream()
    rng = np.random.default_rng(55)

    def unit(n, alphabet):
        return np.frombuffer(alphabet, np.uint8)[rng.integers(0, len(alphabet), size=n)].tobytes()

    quals = bytes(range(35, 74))
    if part == "a":
        cases = [(n, d) for d in range(1, 10) for n in list(range(3, 21)) + [258]]
    else:
        cases = [(n, d) for d in range(8, 64) for n in (d + 1, 258)]
        cases += [(n, n + k) for n in (63, 64, 65, 66, 127, 128, 129, 130, 258) for k in (0, 1, 7, 13)]
        cases += [(n, n + k) for n in (67, 68, 69, 70) for k in (0, 7)]  # (the tails of 3..6 bytes the listed lengths leave out)
    for i, (n, d) in enumerate(cases):
        def line(alphabet):
            def go():
                s.lit(unit(d, alphabet))
                s.match(n, d)
            return go
        _rec(s, b"s%d" % i, line(b"ACGT"), line(quals))
        if i % 40 == 39:
            s.end_block("fixed" if i % 80 == 79 else "dynamic")
    return _case("A5" + part, s)


def a6_chains():
    """records of 64 bytes repeated: in fixed blocks (no literal pairs: a group of 64 tokens is 64 symbols of the queue) 64
    literals, then matches of 16 at distance 64 -- every group of 64 tokens writes exactly 1 024 bytes --, then of 32 (2 048 a
    group), then (64, 64): each match's source is the output of the token before it; the last again under a dynamic code"""
    s = Stream()
    rng = np.random.default_rng(56)
    rec = b"@ab\n" + np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, size=28)].tobytes() + b"\n+\n" + bytes(rng.integers(35, 74, size=28, dtype=np.uint8)) + b"\n"
    assert len(rec) == 64
    s.lit(rec)
    for n in (16, 32, 64):
        for _ in range(192):  # three groups of 64 tokens each, whole records
            s.match(n, 64)
    s.end_block("fixed")
    for _ in range(200):
        s.match(64, 64)
    s.end_block("dynamic")
    s.feed(fastq_text(30, 57), "nearest")  # (text with k-mers in it, so that the sketch has something to say)
    s.feed(rec * 150, "chain", max_len=64)
    return _case("A6", s)


def a4_headers():
    """one block per header shape (its `tag` names it); the stats of each block carry the fields the census reads"""
    s = Stream()
    text = fastq_text(80, 54)
    cut = record_cuts(text, 9)
    # every symbol at 8 bits: the code-length code needs 16, 17, 18, 0 and 8 alone -- HCLEN 5, the least a block with an
    # end-of-block code can have (with HCLEN 4 every length is 0: that one is among the refused); HLIT 257, HDIST 1 of length 0
    s.feed(text[cut[0]:cut[1]], "none")
    s.end_block(ll=[0] + [8] * 256, dl=[0], tag="hclen5")
    s.feed(text[cut[1]:cut[2]], "none")
    s.end_block(hclen=19, tag="hclen19")
    # one distance code of length 1: symbol 0 (a run of one quality value), then symbol 29 (text from 30 000 bytes back)
    s.feed(b"@run/1\nACGTACGTACGTACGTACGTACGT\n+\n", "none")
    s.lit(b"I")
    s.match(23, 1)
    s.lit(b"\n")
    s.end_block(tag="dist_sym0")
    far = fastq_exact(30000, 59)
    s.feed(far, "none")
    s.end_block()
    s.feed(far[:record_cuts(far, 8)[1]], "farthest", max_dist=30000, min_len=100)
    s.end_block(tag="dist_sym29")
    # HLIT 286 with HDIST 30, and a run of eight 9s from the literal/length lengths into the distance lengths: a 16 across HLIT
    s.feed(text[cut[2]:cut[3]], "nearest")
    s.end_block(hlit=286, hdist=30, ll_force={x: 9 for x in range(281, 286)}, dl_force={0: 9, 1: 9, 2: 9}, tag="full_16_cross")
    # trailing zero lengths sent on purpose, a distance code whose first symbols are unused: an 18 run across HLIT; and
    # literals 115..255 unused: code 18 with 138 zeros
    s.feed(text[cut[3]:cut[4]], "nearest", min_len=8, max_len=100)
    s.end_block(hlit=280, tag="18_cross")
    s.feed(text[cut[4]:cut[5]], "nearest", min_len=12, max_len=100)
    s.end_block(hlit=280, cross=False, tag="no_cross")
    # seven equal lengths in a row: code 16 with 6 repeats
    s.feed(text[cut[5]:cut[6]], "none")
    s.end_block(ll_force={x: 9 for x in range(97, 104)}, tag="16x6")
    s.feed(text[cut[6]:cut[7]], "nearest")
    s.end_block(runs=False, tag="no_runs")
    s.feed(text[cut[7]:], "nearest")
    return _case("A4", s)


def a7_blocks():
    s = Stream()
    text = fastq_text(160, 60)
    cut = record_cuts(text, 6)
    s.feed(text[cut[0]:cut[1]], "nearest")
    s.end_block()
    s.end_block("fixed", tag="empty")           # empty blocks in the middle
    s.end_block("dynamic", tag="empty")
    s.stored(b"", tag="stored0")
    # a stored block behind a block that ends at each bit phase: small blocks of growing size until all eight have been seen
    piece, at = text[cut[1]:cut[2]], 0
    for i in range(48):
        n = 30 + i
        s.feed(piece[at:at + n], "nearest")
        at += n
        s.end_block("fixed" if i % 3 == 0 else "dynamic", tag="before_stored")
        s.stored(piece[at:at + 11], tag="stored_small")
        at += 11
    s.feed(piece[at:], "nearest")
    s.end_block()
    # >= 200 consecutive blocks of fewer than 64 symbols
    s.feed(text[cut[2]:cut[3]], "nearest")
    s.cut_blocks(15, tag="tiny")
    s.feed(text[cut[3]:cut[4]], "nearest")
    s.end_block()
    # a block of matches only: text that has been seen, spelled as matches of 258 and a rest
    again = text[cut[3]:cut[3] + record_cuts(text[cut[3]:cut[4]], 3)[1]]
    assert bytes(s.text) == text[:cut[4]]
    d = cut[4] - cut[3]
    for i in range(0, len(again), 258):
        s.match(min(258, len(again) - i), d) if len(again) - i >= 3 else s.lit(again[i:])
    s.end_block(tag="matches_only")
    s.feed(text[cut[4]:cut[5]], "nearest")
    s.end_block()
    s.end_block("dynamic", tag="empty")
    s.blocks.append(Block("fixed", [], final=True, tag="empty"))  # an empty block as the final one
    return _case("A7", s)


def a7_empty_dynamic_last():
    s = Stream()
    s.feed(fastq_text(40, 61), "nearest")
    s.end_block("fixed")
    s.blocks.append(Block("dynamic", [], final=True, tag="empty"))
    return _case("A7e", s)


def a7_stored_65535():
    """a stored block of 65 535 bytes and one literal: 65 536 bytes of text whose last token starts at 65 535 (more DEFLATE
    bytes than a BGZF header can announce: for the member table of the device push and for plain gzip)"""
    s = Stream()
    text = fastq_exact(65536, 62)
    s.stored(text[:65535], tag="stored65535")
    s.lit(text[65535:])
    s.end_block("fixed")
    return _case("A7s", s, bgzf=False)


def a7_member_sizes():
    """BGZF members of 1, 0 and 65 536 bytes of text -- together one FASTQ file; the last one's final token is a literal at 65 535"""
    out = []
    text = fastq_exact(65537, 63)
    one = Stream()
    one.lit(text[:1])
    one.end_block("fixed")
    out.append(_case("A7m1", one, fastq=False))
    e = Stream()
    e.end_block("fixed")
    out.append(_case("A7m0", e, fastq=False))
    full = Stream()
    full.feed(text[1:-1], "nearest", max_cand=4)
    full.lit(text[-1:])
    out.append(_case("A7m65536", full, fastq=False))
    assert isinstance(out[2].blocks[-1].tokens[-1], int) and len(out[2].text) == 65536
    return out


def a8_literal_pairs():
    """the literal/length table's index is 10 bits: two literals whose code lengths sum to 10 share an entry, to 11 do not; a
    literal followed within the index by the end-of-block code or by a length symbol must not be read as a pair.  Blocks of
    two records, each ending literal, end-of-block."""
    s = Stream()
    text = fastq_text(150, 64)
    recs = text.split(b"\n")
    n_rec = len(recs) // 4
    lsym_force = None
    for r0 in range(0, n_rec, 2):
        chunk = b"\n".join(recs[4 * r0:4 * (r0 + 2)]) + b"\n"
        s.feed(chunk[:-1], "nearest", min_len=6, max_cand=4)
        s.lit(b"\n")
        if lsym_force is None:
            lf, _ = _histogram(s.cur, False)
            lsym_force = max(range(257, 286), key=lambda x: (lf[x], -x))
        force = {ord("A"): 5, ord("C"): 5, ord("T"): 5, ord("G"): 6, ord("\n"): 4, EOB: 3, lsym_force: 4}
        s.end_block(ll_force=force)
    return _case("A8", s)


def a9_gzip_headers(text_seed=65):
    """(name, gzip image, text): FEXTRA, FNAME, FCOMMENT and FHCRC together and each alone, around one small stream"""
    s = Stream()
    s.feed(fastq_text(120, text_seed), "nearest")
    c = _case("A9", s)
    fields = dict(fextra=b"XY\x04\x00abcd", fname=b"reads.fastq", fcomment=b"a comment", fhcrc=True)
    out = [("all", gzip_container(c.raw, c.text, **fields))]
    for k, v in fields.items():
        out.append((k, gzip_container(c.raw, c.text, **{k: v})))
    return c, out


def long_periodic():
    """plain gzip only: 8 periods of 32 768; in every period after the first the first 12 KiB are matches at distance 32 768
    (a byte of period 0 is carried through seven windows), the rest literals -- blocks of 900 tokens"""
    s = Stream()
    p0 = fastq_exact(P, 66)
    s.feed(p0, "none")
    for _ in range(7):
        s.feed(p0[:12288], "farthest")
        s.feed(p0[12288:], "none")
    s.cut_blocks(900)
    return _case("L1", s, bgzf=False)


def long_chain():
    """plain gzip only: literal records, then one record whose sequence line is 16 bases repeated 1 200 times, spelled
    (16, 16) -- every match reads the output of the one before it -- under codes of 15 bits for the length and the distance
    symbol (some 4 bytes a token: the chain crosses more than four chunks of 1 024 bytes), in blocks of 600 tokens"""
    s = Stream()
    rng = np.random.default_rng(68)
    text = fastq_text(560, 67)
    cut = record_cuts(text, 8)
    s.feed(text[:cut[7]], "none")
    unit = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, size=16)].tobytes()
    s.lit(b"@long/68\n" + unit)
    s.cut_blocks(800)
    for _ in range(1200):
        s.match(16, 16)
    ll, dl = [0] * 286, [0] * 30
    for i in range(1, 15):  # (unused symbols take the rest of the code space: the codes are complete)
        ll[i], dl[7 + i] = i, i
    ll[EOB] = ll[length_symbol(16)[0]] = dl[distance_symbol(16)[0]] = dl[22] = 15
    s.cut_blocks(600, ll=ll, dl=dl)
    s.feed(b"\n+\n" + bytes(rng.integers(35, 74, size=16 * 1201, dtype=np.uint8)) + b"\n" + text[cut[7]:], "none")
    s.cut_blocks(800)
    return _case("L2", s, bgzf=False)


def _prefix():
    """the valid start of every refused stream: one small non-final block"""
    s = Stream()
    s.feed(fastq_text(3, 70), "nearest")
    s.end_block("fixed")
    return s


def refused_streams():
    """[(id, raw DEFLATE bytes, text)]: zlib refuses each.  `text` is what the tokens spell -- what a decoder that overlooks the
    fault would write, so that a container's CRC-32 and size cannot do the refusing for it -- or b"" where they spell nothing"""
    out = []

    def spelled(blocks):
        try:
            return tokens_text(blocks)
        except (TypeError, ValueError, IndexError):
            return b""

    def add(cid, *blocks, prefix=None):
        s = prefix or _prefix()
        for b in blocks:
            s.blocks.append(b)
        s.blocks[-1].final = True
        out.append((cid, write_stream(s.blocks), spelled(s.blocks)))

    # (one FASTQ record either way, so that a decoder that overlooks the fault hands the splitter valid text)
    lits = list(b"@r/9\nACGTACGTTTGACA\n+\nIIIIIIIIIIIIII\n")
    with_m = list(b"@r/9\nACGTACGTTTGACA\n+\nI") + [(5, 1)] + list(b"JJ") + [(4, 7)] + list(b"KK\n")  # distance symbols 0 and 5
    nat = fit_lengths(_histogram(lits, False)[0])  # a complete literal/length code for `lits`
    one_longer = list(nat)
    one_longer[ord("A")] += 1
    one_shorter = list(nat)
    short = max(range(257), key=lambda x: nat[x])
    one_shorter[short] -= 1
    used = sorted(set(lits) | {EOB})  # twelve symbols: four codes of 3 bits and eight of 4
    ll34 = [0] * 257
    for i, x in enumerate(used):
        ll34[x] = 3 if i < 4 else 4
    assert len(used) == 12

    def cl_code(l0, l34, l17, l18):  # the code-length code for ll34: symbols 0, 3, 4, 17, 18
        c = [0] * 19
        c[0], c[3], c[4], c[17], c[18] = l0, l34, l34, l17, l18
        return c

    add("R_ll_incomplete", Block("dynamic", lits, ll=one_longer))
    add("R_dist_incomplete", Block("dynamic", with_m, dl=[2, 0, 0, 0, 0, 2]))
    add("R_cl_incomplete", Block("dynamic", lits, cl_lens=cl_code(2, 3, 3, 2), ll=ll34))
    add("R_ll_oversubscribed", Block("dynamic", lits, ll=one_shorter))
    add("R_dist_oversubscribed", Block("dynamic", with_m, dl=[1, 1, 0, 0, 0, 1]))
    add("R_cl_oversubscribed", Block("dynamic", lits, cl_lens=cl_code(1, 2, 2, 2), ll=ll34))
    add("R_hlit_30", Block("dynamic", lits, hlit=287))  # (the field: HLIT - 257; 287 and 288 lengths are really sent)
    add("R_hlit_31", Block("dynamic", lits, hlit=288))
    add("R_hdist_31", Block("dynamic", with_m, hdist=31))
    add("R_hdist_32", Block("dynamic", with_m, hdist=32))
    # the length sequence spelled out: code 16 first / a run beyond HLIT + HDIST
    cl = [0] * 19
    for x in (0, 3, 16, 18):
        cl[x] = 2
    add("R_16_first", Block("dynamic", [], cl_lens=cl, cl_syms=[(16, 0), (3, 0), (18, 127), (18, 105)], hlit=257, hdist=1, ll=[3] * 257))
    add("R_run_overruns", Block("dynamic", [], cl_lens=cl, cl_syms=[(3, 0), (18, 127), (18, 127), (3, 0)], hlit=257, hdist=1, ll=[3] * 257))
    no_eob = list(fit_lengths([1 if x in (65, 67, 71, 84) else 0 for x in range(257)]))
    add("R_no_eob", Block("dynamic", list(b"ACGT"), ll=no_eob, eob=False))
    add("R_hclen_4", Block("dynamic", [], cl_lens=[1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1], cl_syms=[(18, 127), (18, 109)], ll=[0] * 257, hlit=257, hdist=1,
                           hclen=4, eob=False))
    add("R_fixed_sym_286", Block("fixed", lits + [("L", 286)] + lits))
    add("R_fixed_sym_287", Block("fixed", lits + [("L", 287)] + lits))
    add("R_fixed_dist_30", Block("fixed", lits + [("M", 5, 30, 77)] + lits))
    add("R_fixed_dist_31", Block("fixed", lits + [("M", 5, 31, 0)] + lits))
    # a distance one byte beyond the start of the stream: in the first block, and behind 31 000 bytes of text (the furthest
    # back a distance code can still miss the start: after 32 768 bytes every distance lands inside the stream)
    first = Stream()
    first.lit(b"@r\nACGT")
    first.cur.append((4, 8))
    first.text += b"ACGT"
    first.lit(b"\n+\nIIIIIIII\n")
    first.end_block("fixed", final=True)
    out.append(("R_far_first_block", write_stream(first.blocks), b""))
    late = Stream()
    late.feed(fastq_exact(31000, 71), "nearest", max_cand=2)
    late.end_block()
    late.lit(b"@r\nACGT")
    late.cur.append((4, len(late.text) + 1))
    late.text += b"ACGT"
    late.lit(b"\n+\nIIIIIIII\n")
    late.end_block("fixed", final=True)
    assert len(late.text) < 32768  # (the distance fits a distance code: it is the START of the text that it misses)
    out.append(("R_far_after_31k", write_stream(late.blocks), b""))
    add("R_btype_3", Block("fixed", lits, btype=3))
    add("R_stored_nlen", Block("stored", data=b"@r\nACGT\n+\nIIII\n", nlen=0x1234))
    return out


class Corpus:
    pass


@functools.lru_cache(maxsize=None)
def corpus():
    c = Corpus()
    c.a9, c.a9_images = a9_gzip_headers()
    c.accepted = [a1_far_distances(), a2_long_codes(), a3_258_as_284(), a4_headers(), a5_copy_match_seams("a"), a5_copy_match_seams("b"), a6_chains(), a7_blocks(),
                  a7_empty_dynamic_last(), a7_stored_65535()] + a7_member_sizes() + [a8_literal_pairs(), c.a9]
    c.long = [long_periodic(), long_chain()]
    c.refused = refused_streams()
    c.by_id = {x.id: x for x in c.accepted + c.long}
    return c
