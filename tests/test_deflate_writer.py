"""tests/deflate_writer.py against zlib, and a census of its corpus.  The writer exists to reach the parts of RFC 1951 that
zlib's own encoder never writes; what it writes is only worth feeding the decoders if zlib's INFLATE agrees with the
verdict the corpus claims (text reproduced / stream refused), and if every shape the corpus is named after is really in
it -- counted here from the token and header lists, so that a later edit cannot hollow the corpus out."""
import collections
import gzip
import zlib

import pytest

import deflate_writer as W


@pytest.fixture(scope="module")
def corpus():
    return W.corpus()


def zlib_inflate(raw):
    d = zlib.decompressobj(-15)
    out = d.decompress(raw)
    assert d.eof and d.unused_data == b""
    return out


def matches(case):
    return [t for t in case.tokens() if not isinstance(t, int)]


def test_zlib_inflates_every_accepted_stream_to_its_text(corpus):
    for c in corpus.accepted + corpus.long:
        assert zlib_inflate(c.raw) == c.text, c.id
        assert len(c.text) <= 256 * 1024, c.id
        if c.bgzf:  # one BGZF member holds it
            assert len(c.text) <= 65536 and len(c.raw) + 26 <= 65536, c.id
    ids = [c.id for c in corpus.accepted]
    assert len(set(ids)) == len(ids)


def test_zlib_refuses_every_refused_stream(corpus):
    want = {"R_ll_incomplete", "R_dist_incomplete", "R_cl_incomplete", "R_ll_oversubscribed", "R_dist_oversubscribed", "R_cl_oversubscribed",
            "R_hlit_30", "R_hlit_31", "R_hdist_31", "R_hdist_32", "R_16_first", "R_run_overruns", "R_no_eob", "R_hclen_4", "R_fixed_sym_286",
            "R_fixed_sym_287", "R_fixed_dist_30", "R_fixed_dist_31", "R_far_first_block", "R_far_after_31k", "R_btype_3", "R_stored_nlen"}
    assert {cid for cid, _, _ in corpus.refused} == want
    for cid, raw, _ in corpus.refused:
        with pytest.raises(zlib.error):
            zlib.decompressobj(-15).decompress(raw)
    # the fault is the stream's only one: its valid prefix alone inflates
    prefix = W._prefix()
    raw, text = prefix.finish()
    assert zlib_inflate(raw) == text and len(text) > 0


def test_what_zlib_accepts_of_incomplete_codes(corpus):
    """the rule the decoders follow (inflate): one code of length 1 in the literal/length or the distance code, or no
    distance code at all -- nothing else that leaves code space unused"""
    lits = list(b"@r\nACGT\n+\nIIII\n")
    for dl in ([1], [0] * 29 + [1], [0]):
        b = W.Block("dynamic", lits, dl=dl, final=True)
        assert zlib_inflate(W.write_stream([b])) == bytes(lits)
    only_eob = W.Block("dynamic", [], final=True)  # a literal/length code of one code: the end-of-block symbol at length 1
    W.write_stream([only_eob])
    assert only_eob.stats["ll"][256] == 1 and sum(only_eob.stats["ll"]) == 1
    assert zlib_inflate(W.write_stream([only_eob])) == b""
    for dl in ([2, 2], [2], [1, 0, 2]):
        with pytest.raises(zlib.error):
            zlib_inflate(W.write_stream([W.Block("dynamic", lits, dl=dl, final=True)]))


def test_a1_holds_the_distances_zlib_never_writes(corpus):
    c = corpus.by_id["A1"]
    m = matches(c)
    far = [(n, d) for n, d in m if 32507 <= d <= 32767]
    top = [(n, d) for n, d in m if d == 32768]
    assert len(far) >= 64 and len(top) >= 64
    assert sum(1 for n, _ in top if n == 3) >= 64 and sum(1 for n, _ in top if n == 258) >= 16
    assert sum(1 for n, _ in far if n == 3) >= 64 and any(n == 258 for n, _ in far)
    assert len({d for _, d in far}) >= 64  # (spread over the range, not one value)
    # ... and why the case exists: zlib's own best effort on the same text stops at MAX_DIST = 32768 - 262
    co = zlib.compressobj(9, zlib.DEFLATED, -15, 9)
    own, n_lit = W.read_tokens(co.compress(c.text) + co.flush())
    assert n_lit + sum(n for n, _ in own) == len(c.text)
    assert len(own) > 1000 and max(d for _, d in own) <= 32506


def test_a2_decodes_through_every_long_code_class(corpus):
    c = corpus.by_id["A2"]
    ll, dl, eob = collections.Counter(), collections.Counter(), set()
    for b in c.blocks:
        for k, v in b.stats["ll_used"].items():
            ll[k] += v
        for k, v in b.stats["dl_used"].items():
            dl[k] += v
        eob.add(b.stats["eob_len"])
        assert max(b.stats["cl_lens"]) == 7
        assert any(b.stats["cl_lens"][s] == 7 for s, _ in b.stats["cl_syms"])  # a 7-bit code that is used
    for bits in range(11, 16):  # beyond the device's 10-bit and the host's 11-bit index (11: the device's alone)
        assert ll[("lit", bits)] >= 64 and ll[("len", bits)] >= 64, bits
    assert eob == {11, 12, 13, 14, 15}
    for bits in range(9, 16):   # beyond both 8-bit distance indexes
        assert dl[bits] >= 64, bits


def test_a3_spells_258_as_284_plus_31(corpus):
    c = corpus.by_id["A3"]
    assert all(b.opts.get("as_284") for b in c.blocks)
    assert sum(1 for n, _ in matches(c) if n == 258) >= 64
    assert W.length_symbol(258, True) == (284, 5, 31) and W.length_symbol(257) == (284, 5, 30)


def _runs_across_hlit(st):
    """code-length symbols of a header whose run begins among the literal/length lengths and ends among the distance lengths"""
    at, out = 0, []
    for s, extra in st["cl_syms"]:
        n = 1 if s < 16 else (3 if s < 18 else 11) + extra
        if s >= 16 and at < st["hlit"] < at + n:
            out.append(s)
        at += n
    assert at == st["hlit"] + st["hdist"]
    return out


def test_a4_headers_have_the_fields_they_are_named_after(corpus):
    c = corpus.by_id["A4"]
    by_tag = {b.opts["tag"]: b.stats for b in c.blocks if "tag" in b.opts}
    st = by_tag["hclen5"]
    assert (st["hclen"], st["hlit"], st["hdist"], st["dl"]) == (5, 257, 1, [0]) and set(st["ll"][1:]) == {8}
    st = by_tag["hclen19"]
    assert (st["hclen"], st["hlit"], st["hdist"], st["dl"]) == (19, 257, 1, [0])
    st = by_tag["dist_sym0"]
    assert st["dl"] == [1] and st["hdist"] == 1 and sum(st["dl_used"].values()) == 1
    st = by_tag["dist_sym29"]
    assert st["dl"] == [0] * 29 + [1] and st["hdist"] == 30 and sum(st["dl_used"].values()) >= 8
    st = by_tag["full_16_cross"]
    assert (st["hlit"], st["hdist"]) == (286, 30) and _runs_across_hlit(st) == [16]
    assert (16, 3) in st["cl_syms"]  # six repeats
    st = by_tag["18_cross"]
    assert _runs_across_hlit(st) == [18] and (18, 127) in st["cl_syms"] and st["hdist"] > 1  # 138 zeros
    st = by_tag["no_cross"]
    assert _runs_across_hlit(st) == [] and st["hdist"] > 1 and any(s >= 16 for s, _ in st["cl_syms"])
    st = by_tag["16x6"]
    assert (16, 3) in st["cl_syms"] and st["ll"][97:104] == [9] * 7
    st = by_tag["no_runs"]
    assert all(s < 16 for s, _ in st["cl_syms"]) and len(st["cl_syms"]) == st["hlit"] + st["hdist"]


def test_a5_sits_on_the_seams_of_copy_match(corpus):
    a, b = matches(corpus.by_id["A5a"]), matches(corpus.by_id["A5b"])
    replay = collections.Counter((n, d) for n, d in a if d <= 9)
    for d in range(1, 10):
        for n in list(range(3, 21)) + [258]:
            assert replay[(n, d)] >= 2, (n, d)
    assert sum(replay.values()) >= 64
    overlap = [(n, d) for n, d in b if 8 <= d <= 63 and n > d]
    assert len(overlap) >= 64 and {d for _, d in overlap} == set(range(8, 64))
    apart = collections.Counter(n for n, d in b if d >= n and n in (63, 64, 65, 66, 67, 68, 69, 70, 127, 128, 129, 130, 258))
    assert sum(apart.values()) >= 64 and all(apart[n] >= 8 for n in (63, 64, 65, 66, 127, 128, 129, 130)), apart
    assert {n % 8 for n in apart} == set(range(8))  # every tail of 1..7 bytes, and none


def test_a6_chains_and_group_sizes(corpus):
    c = corpus.by_id["A6"]
    toks = c.tokens()
    best = run = 0
    prev = 1
    for t in toks:
        if not isinstance(t, int) and t[1] <= prev:  # its source lies inside what the token before it wrote
            run += 1
            best = max(best, run)
        else:
            run = 0
        prev = 1 if isinstance(t, int) else t[0]
    assert best >= 64
    # the first block is fixed (no literal pairs): groups of 64 tokens as the kernels queue them
    first = c.blocks[0]
    assert first.kind == "fixed"
    sizes = [sum(1 if isinstance(t, int) else t[0] for t in first.tokens[i:i + 64]) for i in range(0, len(first.tokens) - 63, 64)]
    assert sizes.count(1024) >= 3 and sizes.count(2048) >= 3 and sizes.count(4096) >= 3 and sizes[0] == 64


def test_a7_block_census(corpus):
    c = corpus.by_id["A7"]
    tags = collections.Counter((b.kind, b.opts.get("tag")) for b in c.blocks)
    assert tags[("fixed", "empty")] >= 2 and tags[("dynamic", "empty")] >= 2 and tags[("stored", "stored0")] == 1
    assert c.blocks[-1].kind == "fixed" and c.blocks[-1].tokens == [] and c.blocks[-1].final
    phases = {b.stats["end_bit"] % 8 for i, b in enumerate(c.blocks[:-1]) if b.kind != "stored" and c.blocks[i + 1].kind == "stored"}
    assert phases == set(range(8))
    run = best = 0
    for b in c.blocks:
        run = run + 1 if b.kind != "stored" and 0 < len(b.tokens) < 64 else 0
        best = max(best, run)
    assert best >= 200
    only = [b for b in c.blocks if b.opts.get("tag") == "matches_only"]
    assert len(only) == 1 and len(only[0].tokens) >= 8 and not any(isinstance(t, int) for t in only[0].tokens)
    last = corpus.by_id["A7e"].blocks[-1]
    assert last.kind == "dynamic" and last.tokens == [] and last.final
    big = corpus.by_id["A7s"]
    assert [len(b.data) for b in big.blocks if b.kind == "stored"] == [65535] and len(big.text) == 65536
    assert [len(corpus.by_id[i].text) for i in ("A7m0", "A7m1", "A7m65536")] == [0, 1, 65536]
    assert [c.id for c in corpus.accepted if not c.fastq] == ["A7m1", "A7m0", "A7m65536"]
    assert isinstance(corpus.by_id["A7m65536"].blocks[-1].tokens[-1], int)  # a token that starts at 65 535


def test_a8_literal_pairs_on_both_sides_of_the_index(corpus):
    c = corpus.by_id["A8"]
    p = collections.Counter()
    for b in c.blocks:
        for k, v in b.stats["pairs"]["lit_lit"].items():
            p[k] += v
        p["len"] += b.stats["pairs"]["lit_len"]
        p["eob"] += b.stats["pairs"]["lit_eob"]
    assert p[10] >= 64 and p[11] >= 64 and p["len"] >= 64 and p["eob"] >= 64


def test_a9_gzip_headers(corpus):
    names = [n for n, _ in corpus.a9_images]
    assert names == ["all", "fextra", "fname", "fcomment", "fhcrc"]
    for name, img in corpus.a9_images:
        assert gzip.decompress(img) == corpus.a9.text, name
    assert corpus.a9_images[0][1][3] == 4 | 8 | 16 | 2


def test_the_long_streams_are_long(corpus):
    for c in corpus.long:
        assert len(c.raw) >= 64 * 1024 and len(c.text) <= 256 * 1024
        sizes = sorted(len(b.tokens) for b in c.blocks)
        assert sizes[len(sizes) // 10] >= 600, c.id  # (the last block of a stretch may be shorter)
    per = corpus.by_id["L1"]
    assert per.text[:W.P] * 8 == per.text
    assert sum(1 for n, d in matches(per) if d == W.P) >= 7 * 40
    chain = matches(corpus.by_id["L2"])
    assert len(chain) == 1200 and set(chain) == {(16, 16)}
    spent = sum(b.stats["end_bit"] - b.stats["start_bit"] for b in corpus.by_id["L2"].blocks if b.tokens and not isinstance(b.tokens[0], int))
    assert spent >= 4 * 1024 * 8  # the chain's own DEFLATE bytes span more than four chunks of 1 024


def test_bgzf_and_gzip_containers_are_what_other_readers_expect(corpus):
    c = corpus.by_id["A5a"]
    assert gzip.decompress(W.bgzf_image([(c.raw, c.text), (c.raw, c.text)])) == c.text * 2
    assert gzip.decompress(W.gzip_container(c.raw, c.text)) == c.text
