"""Sort, mark duplicates and index a BAM or SAM of any aligner, host form: bmh_bam_post_file_host through bwamem_hip.bam against a model of
the new rules written here -- templates by name, the bin rule, the 0x400 clear, the header rule -- on a case table; against bam_sorted_file on the golden SAM sets
(byte for byte: file, index, counts, coverage); independence of batch_bytes, the sort window and spilling; the refusals word for word; and csrc/bam_post_core.h
with the host heads / check path as plain C++ under AddressSanitizer and UBSan (tests/bam_post_core_host.cpp).  No device is needed."""
import io
import os
import struct
import subprocess

import numpy as np
import pytest

from test_bam_core import golden_sam_texts, reg2bin
from test_bam_dup import end_word, flag_of, name_of, pair, rec, score_of, set_dup
from test_bam_sort import CONTIGS, BamFile, check_file, fields, golden_streams, make_record, py_sort, split_records

HERE = os.path.dirname(os.path.abspath(__file__))
HEADER = "@HD\tVN:1.0\tSO:unsorted\n" + "".join(f"@SQ\tSN:{n}\tLN:{l}\n" for n, l in CONTIGS) + "@CO\tkept verbatim\n"
BATCHES, WINDOWS = (1, 200, 4096, None), (1, 7, 0)


# ---------------------------------------------------------------------------------------------------------------- files and the tool

def bam_file(path, header_text, contigs, stream, level=1, member=None):
    """an unsorted BAM: header and records as BGZF members (member: the text bytes of a member, so that records straddle members) and the end-of-file member"""
    from bwamem_hip.lib import bam_header, bgzf_compress, bgzf_eof
    data = bam_header(header_text, contigs) + stream
    step = member or len(data) or 1
    with open(path, "wb") as f:
        for a in range(0, len(data), step):
            f.write(bgzf_compress(data[a:a + step], level, host=True))
        f.write(bgzf_eof())
    return str(path)


def post(path, host=True, **kw):
    from bwamem_hip.bam import bam_post_file
    out, ix = io.BytesIO(), io.BytesIO()
    r = bam_post_file(str(path), out, index=ix, host=host, **kw)
    return out.getvalue(), ix.getvalue(), r


# ---------------------------------------------------------------------------------------------------------------- the model

class Refused(Exception):
    pass


def model_header(text: str) -> str:
    return "@HD\tVN:1.6\tSO:coordinate\n" + "".join(l for l in text.splitlines(True) if not (l.rstrip("\r\n") == "@HD" or l.startswith("@HD\t")))


def model_bin(r: bytes) -> int:
    _rid, pos, _b, _fl, end = fields(r)
    return 4680 if pos < 0 else reg2bin(pos, end)


def full_name(r: bytes) -> bytes:
    return r[12:13] + r[36:36 + r[12]]                         # l_read_name and all its bytes


def model_templates(recs) -> list:
    """lists of record indices: maximal runs of adjacent records under one name"""
    out = []
    for i, r in enumerate(recs):
        if i and full_name(r) == full_name(recs[i - 1]):
            out[-1].append(i)
        else:
            out.append([i])
    return out


def model(header_text: str, stream: bytes, markdup: bool):
    """(the output header, the records as the file must hold them in input order, counts: templates, bins_changed, duplicate_flags_cleared, and with markdup the
    marking's eight)"""
    recs = split_records(stream)
    c = dict(records=len(recs), templates=len(model_templates(recs)), bins_changed=0, duplicate_flags_cleared=0)
    out = []
    for r in recs:
        b = model_bin(r)
        c["bins_changed"] += b != fields(r)[2]
        r = r[:14] + struct.pack("<H", b) + r[16:]
        if markdup and flag_of(r) & 0x400:
            c["duplicate_flags_cleared"] += 1
            r = r[:19] + bytes([r[19] & ~0x04 & 0xFF]) + r[20:]
        out.append(r)
    if not markdup:
        return model_header(header_text), out, c, None
    info = []
    tpls = model_templates(out)
    for t in tpls:
        pri = [out[i] for i in t if not flag_of(out[i]) & 0x900]
        paired = any(flag_of(p) & 1 for p in pri)
        if (paired and (len(pri) != 2 or sorted(flag_of(p) & 0xC0 for p in pri) != [0x40, 0x80])) or (not paired and len(pri) != 1):
            raise Refused(t[0])
        words = [end_word(p) for p in pri if not flag_of(p) & 4]
        info.append((len(words), tuple(sorted(words)), sum(score_of(p) for p in pri)))
    best_pair, pair_ends, best_frag = {}, set(), {}
    for o, (k, w, s) in enumerate(info):
        if k == 2:
            best_pair[w] = min(best_pair.get(w, (0, 1 << 40)), (-s, o)); pair_ends.update(w)
        elif k == 1:
            best_frag[w] = min(best_frag.get(w, (0, 1 << 40)), (-s, o))
    m = dict(pairs_examined=0, fragments_examined=0, duplicate_pairs=0, duplicate_fragments=0, records_flagged=0,
             secondary_or_supplementary=sum(1 for r in out if flag_of(r) & 0x900), unmapped_records=sum(1 for r in out if flag_of(r) & 4), templates=len(tpls))
    for o, ((k, w, _s), t) in enumerate(zip(info, tpls)):
        dup = (k == 2 and best_pair[w][1] != o) or (k == 1 and (w[0] in pair_ends or best_frag[w][1] != o))
        m["pairs_examined"] += k == 2; m["fragments_examined"] += k == 1
        m["duplicate_pairs"] += dup and k == 2; m["duplicate_fragments"] += dup and k == 1
        if dup:
            m["records_flagged"] += len(t)
            for i in t:
                out[i] = set_dup(out[i])
    return model_header(header_text), out, c, m


# ---------------------------------------------------------------------------------------------------------------- the case table

def stale(r: bytes, b: int = 0) -> bytes:
    return r[:14] + struct.pack("<H", b) + r[16:]


def sup(name, rid, pos, flag=0x800):
    return rec(name, rid, pos, flag)


def table():
    """(what, records in file order, markdup, must: what the model itself has to say of the case)"""
    T = []
    a, b = pair(b"p", 1, 100, False, 1, 300, True)
    T.append(("read 2 before read 1", [b, a] + pair(b"q", 1, 100, False, 1, 300, True), True, dict(templates=2, duplicate_pairs=1, flagged={b"q"})))
    T.append(("supplementary before primary", [sup(b"s", 1, 900), rec(b"s", 1, 500, 0), rec(b"t", 1, 500, 0, q=20)], True, dict(templates=2, duplicate_fragments=1, flagged={b"t"})))
    T.append(("secondary first", [sup(b"s", 1, 900, 0x100), rec(b"s", 1, 500, 0, q=20), rec(b"t", 1, 500, 0)], True, dict(templates=2, records_flagged=2, flagged={b"s"})))
    T.append(("r1 and r10 adjacent", [rec(b"r1", 1, 10, 0), rec(b"r10", 1, 10, 0), rec(b"r1", 1, 10, 0)], True, dict(templates=3, duplicate_fragments=2)))
    T.append(("names that differ in the last byte", [rec(b"abcdefgh1", 1, 10, 0), rec(b"abcdefgh2", 1, 10, 0), rec(b"abcdefgX2", 1, 99, 0)], True, dict(templates=3, duplicate_fragments=1)))
    T.append(("names of 1 and of 254 bytes", pair(b"x", 1, 5, False, 1, 50, True) + pair(b"y" * 254, 1, 5, False, 1, 50, True) + pair(b"y" * 253 + b"z", 1, 5, False, 1, 50, True), True,
              dict(templates=3, duplicate_pairs=2)))
    T.append(("two adjacent complete templates under one name", pair(b"z", 1, 5, False, 1, 50, True) + pair(b"z", 1, 700, False, 1, 900, True), True, dict(refused=0)))
    T.append(("the same without marking", pair(b"z", 1, 5, False, 1, 50, True) + pair(b"z", 1, 700, False, 1, 900, True), False, dict(templates=1)))
    T.append(("stale bins", [stale(rec(b"a", 1, 30_000, 0), 0), stale(rec(b"b", 0, 1 << 20, 16), 4681), rec(b"c", 1, 5, 0)], False, dict(bins_changed=2)))
    d = set_dup(rec(b"d", 1, 77, 0))
    T.append(("0x400 on input with marking", [d, rec(b"e", 1, 990, 0)], True, dict(duplicate_flags_cleared=1, records_flagged=0)))
    T.append(("0x400 on input without marking", [d, rec(b"e", 1, 990, 0)], False, dict(duplicate_flags_cleared=0, keeps_0x400=True)))
    T.append(("pos -1", [stale(make_record(-1, -1, 4, b"u1", ops=(), l_seq=20), 0), stale(make_record(1, -1, 4, b"u2", ops=(), l_seq=20), 4681), rec(b"m", 1, 5, 0)], True, dict(bins_changed=2)))
    T.append(("an unmapped-only file", [make_record(-1, -1, 4, b"u%d" % i, ops=(), l_seq=30) for i in range(40)], True, dict(templates=40, records_flagged=0)))
    T.append(("a header and no records", [], True, dict(templates=0)))
    rng = np.random.default_rng(3)
    big = []
    for i in range(400):                                       # pairs and fragments on few positions, so that duplicates are many; supplementary lines anywhere in their template
        p1, p2 = int(rng.integers(0, 6)) * 100, 2000 + int(rng.integers(0, 4)) * 100
        if i % 3:
            t = pair(b"big%d" % i, 1, p1, False, 1, p2, True, q=int(rng.integers(10, 40)))
            if i % 5 == 0:
                t.insert(int(rng.integers(0, 3)), sup(b"big%d" % i, 0, 5000 + i))
            if i % 2:
                t.reverse()
        else:
            t = [rec(b"big%d" % i, 1, p1, 16 * int(rng.integers(0, 2)), q=int(rng.integers(10, 40)))]
        big += [stale(r, int(rng.integers(0, 4681))) if i % 7 == 0 else r for r in t]
    T.append(("many templates", big, True, dict(templates=400)))
    T.append(("many templates without marking", big, False, dict(templates=400)))
    return T


def check_must(what, must, recs, c, m):
    for k, v in must.items():
        if k == "flagged":
            assert {name_of(r) for r in recs if flag_of(r) & 0x400} == v, what
        elif k == "keeps_0x400":
            assert any(flag_of(r) & 0x400 for r in recs), what
        elif k != "refused":
            assert (c[k] if k in c else m[k]) == v, (what, k)


def run_case(tmp_path, what, records, markdup, must, host=True, **kw):
    stream = b"".join(records)
    path = bam_file(tmp_path / "in.bam", HEADER, CONTIGS, stream)
    if "refused" in must:
        with pytest.raises(Refused) as e:
            model(HEADER, stream, markdup)
        assert e.value.args[0] == must["refused"], what
        with pytest.raises(ValueError, match=rf"the records under the read name of record {must['refused']}, .* --collate"):
            post(path, host=host, markdup=markdup, **kw)
        return None
    hdr, recs, c, m = model(HEADER, stream, markdup)
    check_must(what, must, recs, c, m)
    bam, bai, r = post(path, host=host, markdup=markdup, **kw)
    placed = all(fields(r)[1] >= 0 for r in recs if fields(r)[0] >= 0)          # (check_file's region queries centre on records that have a position)
    check_file(bam, bai, hdr, CONTIGS, b"".join(recs), what, n_regions=5 if placed else 0)
    got = {k: r["counts"][k] for k in c}
    assert got == c, (what, got, c)
    if markdup:
        assert r["markdup"] == m, (what, r["markdup"], m)
    return bam, bai, r


@pytest.mark.parametrize("case", table(), ids=lambda c: c[0])
def test_host_equals_model(tmp_path, case):
    run_case(tmp_path, *case)


def test_sam_with_a_header_only(tmp_path):
    p = tmp_path / "h.sam"
    p.write_text(HEADER)
    bam, bai, r = post(p, markdup=True)
    check_file(bam, bai, model_header(HEADER), CONTIGS, b"", "header only", n_regions=0)
    assert r["counts"]["records"] == 0 and r["contigs"] == [(n, l) for n, l in CONTIGS]


def _chunk(n):
    import bwamem_hip
    L = bwamem_hip.load_library()
    L.bmh_tune_set(b"BAM_POST_CHUNK", n, 0) if n else L.bmh_tune_set(b"BAM_POST_CHUNK", 0, 1)


@pytest.mark.parametrize("chunk", (37, 100, 333))
def test_records_and_templates_that_straddle_an_inflate_window(tmp_path, chunk):
    """the source is asked for `chunk` bytes at a time and the file's members hold 150 bytes of text: records (about 120 bytes) and templates straddle both kinds of
    window, and every batch_bytes cuts batches inside them"""
    _what, records, _md, _must = [c for c in table() if c[0] == "many templates"][0]
    stream = b"".join(records)
    whole = post(bam_file(tmp_path / "w.bam", HEADER, CONTIGS, stream), markdup=True)
    path = bam_file(tmp_path / "s.bam", HEADER, CONTIGS, stream, member=150)
    try:
        _chunk(chunk)
        for bb in (1, 200, None):
            got = post(path, markdup=True, batch_bytes=bb)
            assert got[0] == whole[0] and got[1] == whole[1] and got[2]["markdup"] == whole[2]["markdup"], (chunk, bb)
            assert bb is None or got[2]["counts"]["batches"] > 1
    finally:
        _chunk(0)


# ---------------------------------------------------------------------------------------------------------------- equality with what exists

def golden_inputs():
    """(what, contigs, header text, the writer's unsorted stream, the SAM record lines) of the golden SAM sets; a set with two adjacent templates under one name is
    left out (at most one may be)"""
    from bwamem_hip.lib import sam_to_bam
    out, left = [], []
    bodies = {w: body for w, _full, body in golden_sam_texts()}
    for what, contigs, _recs in golden_streams():
        body = bodies[what]
        stream, st = sam_to_bam(body, contigs, host=True)
        assert not np.asarray(st).any(), what
        recs = split_records(stream)
        from test_bam_dup import templates_of
        if len(model_templates(recs)) != len(templates_of(recs)):
            left.append(what)
            continue
        out.append((what, contigs, "".join(f"@SQ\tSN:{n}\tLN:{l}\n" for n, l in contigs), bytes(stream), body))
    assert len(left) <= 1, left
    return out


_GOLDEN = []


def golden():
    if not _GOLDEN:
        _GOLDEN.extend(golden_inputs())
    return _GOLDEN


def golden_files(tmp_path, g):
    what, contigs, header, stream, body = g
    sam = tmp_path / "in.sam"
    sam.write_bytes(header.encode() + body)
    return bam_file(tmp_path / "in.bam", header, contigs, stream), str(sam)


@pytest.mark.parametrize("markdup", (False, True))
@pytest.mark.parametrize("index_format", ("bai", "csi"))
def test_equals_the_sorted_file_of_the_same_stream(tmp_path, markdup, index_format):
    from bwamem_hip.lib import bam_sorted_file
    for g in golden():
        what, contigs, header, stream, _body = g
        want = bam_sorted_file("@HD\tVN:1.6\tSO:coordinate\n" + header, contigs, stream, host=True, markdup=markdup, index_format=index_format, coverage={})
        for path in golden_files(tmp_path, g):
            bam, ix, r = post(path, markdup=markdup, index_format=index_format, coverage=io.StringIO())
            assert bam == want[0] and ix == want[1], (what, path)
            assert r["counts"]["bins_changed"] == 0 and r["counts"]["records"] == len(split_records(stream)), what
            if markdup:
                assert r["markdup"] == want[2], what
            for k, v in want[-1].items():
                assert np.array_equal(r["coverage"][k], v), (what, k)


def test_independence_of_batches_windows_and_spilling(tmp_path):
    two = sorted(golden(), key=lambda g: -len(g[3]))[:2]
    for g in two:
        bam_path, sam_path = golden_files(tmp_path, g)
        want = post(bam_path, markdup=True, coverage=io.StringIO())
        for bb in BATCHES:
            for w in WINDOWS:
                got = post(bam_path if w != 7 else sam_path, markdup=True, coverage=io.StringIO(), batch_bytes=bb, sort_window=w)
                # (a window changes where members end, so the bytes of the file and its index are compared per window; the records, flags and counts with all)
                assert BamFile(got[0]).stream == BamFile(want[0]).stream and got[2]["markdup"] == want[2]["markdup"], (g[0], bb, w)
                assert all(np.array_equal(got[2]["coverage"][k], v) for k, v in want[2]["coverage"].items()), (g[0], bb, w)
                ref = post(bam_path, markdup=True, coverage=io.StringIO(), sort_window=w)
                assert got[0] == ref[0] and got[1] == ref[1], (g[0], bb, w)
        spilled = post(bam_path, markdup=True, coverage=io.StringIO(), batch_bytes=4096, sort_mem=1)
        assert spilled[0] == want[0] and spilled[1] == want[1] and spilled[2]["markdup"] == want[2]["markdup"], g[0]


# ---------------------------------------------------------------------------------------------------------------- refusals

def refused(tmp_path, stream, match, header=HEADER, contigs=CONTIGS, **kw):
    path = bam_file(tmp_path / "bad.bam", header, contigs, stream)
    out = io.BytesIO()
    from bwamem_hip.bam import bam_post_file
    with pytest.raises(ValueError, match=match):
        bam_post_file(path, out, host=kw.pop("host", True), **kw)
    assert out.getvalue() == b"", "a refusal before the first byte leaves nothing"


def refusal_cases():
    good = [rec(b"g%d" % i, 1, 10 * i, 0) for i in range(5)]
    cut = bytearray(rec(b"cut", 1, 70, 0)); cut[20:24] = struct.pack("<I", 5000)           # l_seq beyond the block
    short = rec(b"short", 1, 70, 0)[:60]; short = struct.pack("<I", len(short) - 4) + short[4:]
    p1, p2 = pair(b"srt", 1, 100, False, 1, 5000, True)
    sorted_pairs = [p1, pair(b"oth", 1, 200, False, 1, 6000, True)[0], p2, pair(b"oth", 1, 200, False, 1, 6000, True)[1]]
    hard = rec(b"hard", 1, 100, 0, ops=((1 << 27, 5), (1 << 27, 5), (1 << 27, 5), (1 << 27, 5), (1 << 27, 5), (1 << 27, 5), (1 << 27, 5), (1 << 27, 5), (1 << 27, 5), (50, 0)), l_seq=50)
    cg = make_record(1, 10, 0, b"long", ops=((50, 4), (900, 3)), l_seq=50, tag=b"CGBI" + struct.pack("<I", 1) + struct.pack("<I", 50 << 4))
    return dict(
        cut=(b"".join(good) + bytes(cut), r"record 5 is not whole", {}),
        short=(b"".join(good[:2]) + short + good[2], r"record 2 is not whole", {}),
        truncated=(b"".join(good) + rec(b"t", 1, 5, 0)[:-7], r"record 5 is cut: the input ends inside it", {}),
        ref=(b"".join(good[:3]) + make_record(9, 5, 0, b"far") + good[3], r"record 3 names reference 9 and next reference -1 of 5", {}),
        sorted_markdup=(b"".join(sorted_pairs), r"duplicate marking: the records under the read name of record 0, which lie next to each other, are paired and are not one 0x40 and one 0x80 primary "
                                                r"line: marking needs the records of a read name next to each other \(a coordinate-sorted file has them apart: sort it by name first, or realign it "
                                                r"with --collate\)", dict(markdup=True)),
        place=(b"".join(good) + make_record(-1, -1, 0, b"lost"), r"duplicate marking: record 5 is a primary line without 0x4 and has no place \(refID -1, pos -1\)", dict(markdup=True)),
        hard=(b"".join(good) + hard, r"duplicate marking: record 5 has its unclipped 5' end at -1207959452", dict(markdup=True)),
        placeholder=(b"".join(good) + cg, r"record 5 holds the long-CIGAR placeholder", dict(markdup=True)),
        placeholder_cov=(b"".join(good) + cg, r"record 5 holds the long-CIGAR placeholder", dict(coverage=io.StringIO())),
        first_of_two=(b"".join(good[:2]) + make_record(9, 5, 0, b"far") + bytes(cut), r"record 2 names reference 9", {}),
    ), sorted_pairs, cg


@pytest.mark.parametrize("which", sorted(refusal_cases()[0]))
def test_refusals(tmp_path, which):
    stream, match, kw = refusal_cases()[0][which]
    for bb in (None, 1):
        refused(tmp_path, stream, match, batch_bytes=bb, **kw)


def test_what_marking_refuses_a_plain_sort_takes(tmp_path):
    _cases, sorted_pairs, cg = refusal_cases()
    for stream in (b"".join(sorted_pairs), cg + rec(b"g", 1, 5, 0)):
        bam, bai, r = post(bam_file(tmp_path / "ok.bam", HEADER, CONTIGS, stream))
        check_file(bam, bai, model_header(HEADER), CONTIGS, stream, n_regions=3)
    assert BamFile(post(bam_file(tmp_path / "ok.bam", HEADER, CONTIGS, b"".join(sorted_pairs)))[0]).stream == b"".join(sorted_pairs), "a sorted file comes out in its own order"


def test_sam_refusals(tmp_path):
    from bwamem_hip.bam import bam_post_file
    line = "r%d\t0\tchr2\t%d\t60\t10M\t*\t0\t0\tACGTACGTAC\tIIIIIIIIII\n"
    nosq = tmp_path / "nosq.sam"
    nosq.write_text("@HD\tVN:1.6\n@CO\tno references\n" + line % (1, 5))
    with pytest.raises(ValueError, match=r"the SAM header has no @SQ line"):
        bam_post_file(str(nosq), io.BytesIO(), host=True)
    bad = tmp_path / "bad.sam"
    n_header = HEADER.count("\n")
    bad.write_text(HEADER + line % (1, 5) + line % (2, 6) + "r3\t0\tchr2\t7\t60\t10M\t*\t0\t0\tACGTACGTAC\tIIIIIIIIII\tXB:B:c,1,2\n" + line % (4, 8))
    from bwamem_hip.lib import bam_status_name, sam_to_bam
    st = sam_to_bam(b"r3\t0\tchr2\t7\t60\t10M\t*\t0\t0\tACGTACGTAC\tIIIIIIIIII\tXB:B:c,1,2\n", CONTIGS, host=True)[1]
    words = bam_status_name(int(st[0]))
    for bb in (None, 1):
        out = io.BytesIO()
        with pytest.raises(ValueError) as e:
            bam_post_file(str(bad), out, host=True, batch_bytes=bb)
        assert f"line {n_header + 3}: its SAM record cannot be written as BAM: {words}" in str(e.value) and out.getvalue() == b""


def test_option_misuse(tmp_path, capsys):
    from bwamem_hip.bam import bam_post_file, main
    path = bam_file(tmp_path / "in.bam", HEADER, CONTIGS, rec(b"a", 1, 5, 0))
    for kw, words in ((dict(optical_distance=100), "optical_distance needs markdup=True"), (dict(barcode_tag="RX"), "need markdup=True"), (dict(barcode_edits=1), "barcode_edits needs markdup=True"),
                      (dict(libraries=True), "libraries needs markdup=True"), (dict(markdup_metrics=io.StringIO()), "markdup_metrics needs markdup=True"),
                      (dict(coverage_bed=io.StringIO()), "coverage_bed and coverage_bin go together"), (dict(coverage_min_mapq=3), "need coverage, coverage_hist or coverage_bed"),
                      (dict(csi_min_shift=12), 'needs index_format="csi"'), (dict(markdup=True, barcode_tag="RG"), "RG names the read group"), (dict(level=2), "0 or 1"),
                      (dict(batch_bytes=(1 << 30) + 1), "at most 2\\^30"), (dict(markdup=True, libraries=True), "@RG")):
        with pytest.raises(ValueError, match=words):
            bam_post_file(path, io.BytesIO(), host=True, **kw)
    for argv, status, words in ((["--optical-distance", "5", path], 2, "--optical-distance needs --markdup"), (["--libraries", path], 2, "--libraries needs --markdup"),
                                (["--markdup-metrics", "m", path], 2, "--markdup-metrics needs --markdup"), (["--coverage-bed", "b", path], 2, "--coverage-bed and --coverage-bin go together"),
                                (["--csi-min-shift", "12", path], 2, "--csi-min-shift needs --csi"), (["--bam-level", "3", path], 2, "--bam-level needs 0 or 1"),
                                (["--barcode-edits", "1", "--markdup", path], 2, "--barcode-edits needs --barcode-tag or --barcode-name"), (["-C", path], 2, "option -C is not taken"),
                                (["--host", "--markdup", "--libraries", "-o", str(tmp_path / "o.bam"), path], 1, "@RG")):
        assert main(argv) == status
        assert words in capsys.readouterr().err


def test_the_command_and_libraries(tmp_path):
    """the command end to end on the host form: --libraries calls duplicates within a library, the metrics table has a row per library, the index lands beside -o"""
    from bwamem_hip.bam import main
    header = HEADER + "@RG\tID:a\tLB:one\n@RG\tID:b\tLB:two\n@RG\tID:c\tLB:one\n"

    def tagged(r, rg):
        r = r + b"RGZ" + rg + b"\0"
        return struct.pack("<I", len(r) - 4) + r[4:]
    recs = [tagged(rec(b"f1", 1, 100, 0), b"a"), tagged(rec(b"f2", 1, 100, 0, q=20), b"b"), tagged(rec(b"f3", 1, 100, 0, q=10), b"c")]
    path = bam_file(tmp_path / "rg.bam", header, CONTIGS, b"".join(recs))
    o, m = str(tmp_path / "o.bam"), str(tmp_path / "m.txt")
    assert main(["--host", "--markdup", "--libraries", "--markdup-metrics", m, "-o", o, path]) == 0
    f = BamFile(open(o, "rb").read())
    assert [flag_of(r) & 0x400 for r in f.recs] == [0, 0, 0x400] and os.path.getsize(o + ".bai") > 8
    rows = open(m).read().splitlines()[2:]
    assert [r.split("\t")[0] for r in rows] == ["one", "two"] and rows[0].split("\t")[1] == "2" and rows[0].split("\t")[5] == "1"
    assert main(["--host", "--markdup", "--csi", "-o", o, path]) == 0 and os.path.getsize(o + ".csi") > 28
    assert [flag_of(r) & 0x400 for r in BamFile(open(o, "rb").read()).recs] == [0, 0x400, 0x400]


# ---------------------------------------------------------------------------------------------------------------- the core under the sanitizers

def _build():
    out = os.path.join(HERE, "_build"); os.makedirs(out, exist_ok=True)
    exe = os.path.join(out, "bam_post_core_host")
    csrc = os.path.join(HERE, "..", "bwa-mem_gpu_amd", "csrc")
    src = [os.path.join(HERE, "bam_post_core_host.cpp")] + [os.path.join(csrc, f) for f in ("bam_post_core.h", "bam_dup_core.h", "bam_cov_core.h", "bam_dup.h", "bam_dup_host.cpp", "bam_sort_core.h")]
    if not os.path.exists(exe) or any(os.path.getmtime(s) > os.path.getmtime(exe) for s in src):
        subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", src[0], "-o", exe])
    return exe


def test_core_under_sanitizers(tmp_path):
    cases = [(b"".join(records), 1 if markdup else 0) for _w, records, markdup, _m in table()]
    cases += [(stream, 1 | (2 if "coverage" in kw else 0)) for stream, _match, kw in refusal_cases()[0].values()]
    fi, fo = str(tmp_path / "post_case.bin"), str(tmp_path / "post_result.bin")
    with open(fi, "wb") as f:
        f.write(struct.pack("<I", len(cases)) + b"".join(struct.pack("<iIQ", len(CONTIGS), mode, len(s)) + s for s, mode in cases))
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0")
    r = subprocess.run([_build(), fi, fo], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    err = r.stderr.decode(errors="replace")
    assert r.returncode == 0 and "Sanitizer" not in err and "runtime error" not in err, "the sanitizers (or the driver) reported:\n" + err[-4000:]
    res, p = open(fo, "rb").read(), 0
    n_refused = 0
    for stream, mode in cases:
        n = struct.unpack_from("<I", res, p)[0]; p += 4
        recs = []
        q = 0
        while len(stream) - q >= 4 and q + 4 + struct.unpack_from("<I", stream, q)[0] <= len(stream):
            e = q + 4 + struct.unpack_from("<I", stream, q)[0]
            recs.append(stream[q:e]); q = e
        assert n == len(recs)
        codes = []
        for i, rc in enumerate(recs):
            code, bin_, fl, head = struct.unpack_from("<iHHB", res, p); p += 9
            codes.append(code)
            whole = len(rc) >= 36 and len(rc) >= 36 + rc[12] + 4 * struct.unpack_from("<H", rc, 16)[0]
            assert head == (i == 0 or not whole or len(recs[i - 1]) < 36 or full_name(rc) != full_name(recs[i - 1])), i
            if code == 0:
                assert bin_ == model_bin(rc) and fl == (flag_of(rc) & ~0x400 if mode & 1 else flag_of(rc)), i
        st = struct.unpack_from("<i", res, p)[0]; p += 4
        bad = next((i for i, c in enumerate(codes) if c), None)
        if st == 0:
            nt = struct.unpack_from("<I", res, p)[0]; p += 4
            if bad is None:
                assert nt == len(model_templates(recs))
        n_refused += st != 0 or bad is not None
    assert p == len(res) and n_refused >= 8
