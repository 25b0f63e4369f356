"""Mark duplicates in a file that is not grouped by name (BDP_TPL_FILE), host forms: bam_post_file(collate=True) and bam_templates(host=True)
against a model written here -- the records grouped by their full names, the templates ordered by first occurrence, the entries by rule 4 from test_bam_dup's
end_word and score_of, the decision test_bam_dup's model on the templates laid out in the writer's order -- on a case table; byte equality with the option off on
every golden SAM set (name-grouped, distinct names); the golden and synthetic files shuffled, coordinate-sorted and reversed; independence of batch_bytes, the
sort window and spilling; the tool's own output fed back; the refusals word for word; and csrc/bam_tpl_core.h as plain C++ under AddressSanitizer and UBSan
(tests/bam_tpl_core_host.cpp).  No device is needed.

Outputs of two different input orders may differ in the order of records with equal sort keys, so they are compared by record identity: 0x400 per (name, flag
without 0x400, refID, pos), the counts, and check_file on each."""
import io
import os
import struct
import subprocess

import numpy as np
import pytest

from test_bam_core import golden_sam_texts
from test_bam_dup import end_word, flag_of, model as dup_model, name_of, pair, rec, score_of, synthetic
from test_bam_post import BATCHES, HEADER, WINDOWS, Refused, bam_file, full_name, model_bin, model_header, post, sup
from test_bam_sort import CONTIGS, BamFile, check_file, fields, golden_streams, py_sort, split_records

HERE = os.path.dirname(os.path.abspath(__file__))
ONES = (1 << 64) - 1
FOUR = ("pairs_examined", "fragments_examined", "duplicate_pairs", "duplicate_fragments")


# ---------------------------------------------------------------------------------------------------------------- the model

def name_sets(recs) -> list:
    """lists of record indices: the records of the whole file under one full name, the sets in order of first occurrence"""
    sets = {}
    for i, r in enumerate(recs):
        sets.setdefault(full_name(r), []).append(i)
    return list(sets.values())


def primary_lines(recs, t) -> list:
    return [i for i in t if not flag_of(recs[i]) & 0x900]


def proper(recs, t) -> bool:
    pri = [recs[i] for i in primary_lines(recs, t)]
    if any(flag_of(p) & 1 for p in pri):
        return len(pri) == 2 and sorted(flag_of(p) & 0xC0 for p in pri) == [0x40, 0x80]
    return len(pri) == 1


def model_entries(recs):
    """(tpl: every record's ordinal, entries: (lo, hi, score, kind_n) per template) by rule 4; Refused(first index, primary lines, 0x40, 0x80) by rule 5, the
    smallest first index first"""
    sets = name_sets(recs)
    tpl, entries = [0] * len(recs), []
    for o, t in enumerate(sets):
        pri = [recs[i] for i in primary_lines(recs, t)]
        if not proper(recs, t):
            raise Refused(t[0], len(pri), sum(1 for p in pri if flag_of(p) & 1 and flag_of(p) & 0x40), sum(1 for p in pri if flag_of(p) & 1 and flag_of(p) & 0x80))
        words = [end_word(p) for p in pri if not flag_of(p) & 4]
        lo, hi = (min(words), max(words)) if len(words) == 2 else (words[0], ONES) if words else (ONES, ONES)
        entries.append((lo, hi, min(sum(score_of(p) for p in pri), 0xFFFFFFFF), len(words) | len(t) << 2))
        for i in t:
            tpl[i] = o
    return tpl, entries


def collate_model(header_text: str, stream: bytes):
    """(the output header, the records as the file must hold them in input order, the tool's counts, the marking's eight); Refused as model_entries"""
    recs = split_records(stream)
    c = dict(records=len(recs), bins_changed=0, duplicate_flags_cleared=0)
    out = []
    for r in recs:
        b = model_bin(r)
        c["bins_changed"] += b != fields(r)[2]
        r = r[:14] + struct.pack("<H", b) + r[16:]
        if flag_of(r) & 0x400:
            c["duplicate_flags_cleared"] += 1
            r = r[:19] + bytes([r[19] & ~0x04 & 0xFF]) + r[20:]
        out.append(r)
    model_entries(out)
    sets = name_sets(out)
    c["templates"] = len(sets)
    # the writer's order: every template's records next to each other, the primary line that heads a template (unpaired, or 0x40) first; the templates by first occurrence
    laid = []
    for t in sets:
        head = [i for i in primary_lines(out, t) if not flag_of(out[i]) & 1 or flag_of(out[i]) & 0x40][0]
        laid += [head] + [i for i in t if i != head]
    marked, m, _holds = dup_model(b"".join(out[i] for i in laid))
    for i, r in zip(laid, split_records(marked)):
        out[i] = r
    return model_header(header_text), out, c, m


def identity(recs) -> dict:
    """0x400 per (name, flag without 0x400, refID, pos) -- with how many records carry the identity, should two be alike"""
    out = {}
    for r in recs:
        k = (name_of(r), flag_of(r) & ~0x400, fields(r)[0], fields(r)[1])
        out.setdefault(k, []).append(flag_of(r) & 0x400)
    return {k: sorted(v) for k, v in out.items()}


def run(tmp_path, stream, what="", header=HEADER, contigs=CONTIGS, host=True, **kw):
    """the tool with --markdup --collate on the stream against the model: the file and its index (check_file), the counts, the marking's counts"""
    hdr, recs, c, m = collate_model(header, stream)
    bam, bai, r = post(bam_file(tmp_path / "in.bam", header, contigs, stream), host=host, markdup=True, collate=True, **kw)
    placed = all(fields(x)[1] >= 0 for x in recs if fields(x)[0] >= 0)
    check_file(bam, bai, hdr, contigs, b"".join(recs), what, n_regions=5 if placed else 0)
    assert {k: r["counts"][k] for k in c} == c, (what, r["counts"], c)
    assert r["markdup"] == m, (what, r["markdup"], m)
    return bam, bai, r, recs


# ---------------------------------------------------------------------------------------------------------------- the case table

def filler(k, n=3):
    return [rec(b"fill%d_%d" % (k, i), 0, 40_000 + 1000 * k + 10 * i, 0) for i in range(n)]


def table():
    """(what, records in file order, must: the names whose records are flagged)"""
    T = []
    p, q = pair(b"p", 1, 100, False, 1, 300, True), pair(b"q", 1, 100, False, 1, 300, True)
    T.append(("mates apart", [p[0], q[0]] + filler(0) + [p[1]] + filler(1) + [q[1]], {b"q"}))
    T.append(("a supplementary line before and far from its primary", [sup(b"s", 0, 900)] + filler(0) + [rec(b"t", 1, 500, 0, q=20)] + filler(1) + [rec(b"s", 1, 500, 0)], {b"t"}))
    T.append(("read 2 before read 1", [q[1], p[1]] + filler(0) + [p[0], q[0]], {b"p"}))
    T.append(("an unpaired read between the mates of a pair", [p[0], rec(b"u", 1, 100, 0), p[1], rec(b"v", 1, 100, 0)], {b"u", b"v"}))
    h1 = [rec(b"h1", 1, 700, 0x1 | 0x40 | 0x8, q=20), rec(b"h1", 1, 700, 0x1 | 0x80 | 0x4, ops=(), q=20)]
    h2 = [rec(b"h2", 1, 700, 0x1 | 0x40 | 0x8), rec(b"h2", 1, 700, 0x1 | 0x80 | 0x4, ops=())]
    T.append(("a pair with one unmapped mate, placed apart", [h1[1], h2[0]] + filler(0) + [h2[1]] + filler(1) + [h1[0]], {b"h1"}))
    e = pair(b"edge", 1, 5000, False, 1, 5200, True, q=20)
    f = pair(b"mid", 1, 5000, False, 1, 5200, True)
    T.append(("a template at index 0 and index N - 1", [e[0]] + filler(0) + f + filler(1) + [e[1]], {b"edge"}))
    a, b = pair(b"late", 1, 8000, False, 1, 8300, True), pair(b"early", 1, 8000, False, 1, 8300, True)
    T.append(("equal scores: the tie goes to the earlier first record", [sup(b"late", 0, 10)] + b + filler(0) + a, {b"early"}))
    T.append(("the same with the first records in the primaries' order", b + [sup(b"late", 0, 10)] + filler(0) + a, {b"late"}))
    return T


@pytest.mark.parametrize("case", table(), ids=lambda c: c[0])
def test_host_equals_model(tmp_path, case):
    what, records, flagged = case
    stream = b"".join(records)
    _bam, _bai, r, recs = run(tmp_path, stream, what)
    assert {name_of(x) for x in recs if flag_of(x) & 0x400} == flagged, what
    tpl, entries = model_entries(split_records(stream))
    from bwamem_hip.lib import bam_templates
    got = bam_templates(stream, host=True)
    assert got["tpl"].tolist() == tpl and [tuple(int(v) for v in x) for x in got["entries"]] == entries, what
    assert got["counts"]["templates"] == len(entries) == r["markdup"]["templates"], what


def tagged(r: bytes, tags: bytes) -> bytes:
    r = r + tags
    return struct.pack("<I", len(r) - 4) + r[4:]


GROUPS = [("a", "one"), ("b", "two"), ("c", "one")]


def first_record_cases():
    """records that disagree: the read group and the barcode are the earliest record's"""
    from bwamem_hip.lib import barcode_word
    x = pair(b"x", 1, 100, False, 1, 300, True)
    y = pair(b"y", 1, 100, False, 1, 300, True)
    recs = [tagged(x[1], b"RGZb\0RXZACGT\0"), tagged(y[0], b"RGZa\0"), tagged(rec(b"z", 1, 900, 0), b"RGZc\0RXZTT\0")] + [tagged(r, b"RGZc\0") for r in filler(0)] + \
           [tagged(x[0], b"RGZa\0RXZGGGG\0"), tagged(y[1], b"RGZb\0RXZCCCC\0")]
    want_lib = [1, 0, 0, 0, 0, 0]                               # x by its read 2 (b: two), y by its read 1 (a: one), z and the fillers c: one
    want_bc = [barcode_word(b"ACGT"), 0, barcode_word(b"TT"), 0, 0, 0]      # y's first record has no RX: no barcode, though its later record has one
    return b"".join(recs), want_lib, want_bc


def test_read_group_and_barcode_of_the_earliest_record():
    from bwamem_hip.lib import bam_templates
    stream, want_lib, want_bc = first_record_cases()
    got = bam_templates(stream, host=True, read_groups=GROUPS, barcode_tag="RX")
    assert [int(e["lo"]) >> 56 for e in got["entries"]] == want_lib
    assert [int(w) for w in got["barcodes"]] == want_bc
    assert got["libraries"] == {"one": dict(secondary_or_supplementary=0, unmapped_records=0, templates=5), "two": dict(secondary_or_supplementary=0, unmapped_records=0, templates=1)}
    assert [int(l["rg"]) for l in got["locations"]] == [1, 0, 2, 2, 2, 2]


# ---------------------------------------------------------------------------------------------------------------- name-grouped input: the option changes nothing

_GOLDEN = []


def golden_all():
    """(what, contigs, header text, the writer's unsorted stream, the SAM record lines) of every golden SAM set: none is left out"""
    if not _GOLDEN:
        from bwamem_hip.lib import sam_to_bam
        bodies = {w: body for w, _full, body in golden_sam_texts()}
        for what, contigs, _recs in golden_streams():
            stream, st = sam_to_bam(bodies[what], contigs, host=True)
            assert not np.asarray(st).any(), what
            _GOLDEN.append((what, contigs, "".join(f"@SQ\tSN:{n}\tLN:{l}\n" for n, l in contigs), bytes(stream), bodies[what]))
        assert len(_GOLDEN) == 8, [g[0] for g in _GOLDEN]
    return _GOLDEN


def files_of(tmp_path, g):
    what, contigs, header, stream, body = g
    sam = tmp_path / "in.sam"
    sam.write_bytes(header.encode() + body)
    return bam_file(tmp_path / "in.bam", header, contigs, stream), str(sam)


@pytest.mark.parametrize("index_format", ("bai", "csi"))
def test_name_grouped_input_is_byte_for_byte_the_option_off(tmp_path, index_format):
    n = 0
    for g in golden_all():
        recs = split_records(g[3])
        runs = sum(1 for i, r in enumerate(recs) if i == 0 or full_name(r) != full_name(recs[i - 1]))
        assert runs == len(name_sets(recs)) and len(name_sets(recs)) in (300, 600), g[0]
        for path in files_of(tmp_path, g):
            off = post(path, markdup=True, index_format=index_format, coverage=io.StringIO())
            on = post(path, markdup=True, index_format=index_format, coverage=io.StringIO(), collate=True)
            assert on[0] == off[0] and on[1] == off[1], (g[0], path)
            assert on[2]["counts"] == off[2]["counts"] and on[2]["markdup"] == off[2]["markdup"], (g[0], path)
            assert all(np.array_equal(on[2]["coverage"][k], v) for k, v in off[2]["coverage"].items()), (g[0], path)
            n += 1
    assert n == 16, "none of the eight sets is skipped"


# ---------------------------------------------------------------------------------------------------------------- permuted input

def orders(stream: bytes, seed: int) -> dict:
    recs = split_records(stream)
    perm = np.random.default_rng(seed).permutation(len(recs))
    return dict(shuffled=b"".join(recs[i] for i in perm), sorted=py_sort(stream), reversed=b"".join(reversed(recs)))


def permuted_corpus():
    """(what, contigs, header, the name-grouped stream): the two largest golden sets and a synthetic stream of 200 templates"""
    two = sorted(golden_all(), key=lambda g: -len(g[3]))[:2]
    return [(g[0], g[1], g[2], g[3]) for g in two] + [("synthetic 200", CONTIGS, HEADER, synthetic(200, 7))]


@pytest.mark.parametrize("k", range(3))
def test_permuted_input(tmp_path, k):
    what, contigs, header, stream = permuted_corpus()[k]
    grouped = post(bam_file(tmp_path / "g.bam", header, contigs, stream), markdup=True)
    for order, s in orders(stream, 5 + k).items():
        bam, _bai, r, recs = run(tmp_path, s, f"{what} {order}", header=header, contigs=contigs)
        assert {c: r["markdup"][c] for c in FOUR} == {c: grouped[2]["markdup"][c] for c in FOUR}, (what, order)
        assert identity(BamFile(bam).recs) == identity(recs), (what, order)
    # (which member of a duplicate set stays is a matter of the first records' order, which a permutation changes: between orders the counts are equal, the
    # flags need not be; the name-grouped file keeps that order under the option, and its flags)
    assert identity(BamFile(post(bam_file(tmp_path / "g2.bam", header, contigs, stream), markdup=True, collate=True)[0]).recs) == identity(BamFile(grouped[0]).recs), what


def test_the_corpus_holds_duplicates(tmp_path):
    n = 0
    for what, contigs, header, stream in permuted_corpus():
        m = collate_model(header, stream)[3]
        n += m["duplicate_pairs"] + m["duplicate_fragments"]
    assert n > 0 and collate_model(HEADER, synthetic(200, 7))[3]["duplicate_pairs"] > 0


# ---------------------------------------------------------------------------------------------------------------- independence

def test_independence_of_batches_windows_and_spilling(tmp_path):
    what, contigs, header, stream = permuted_corpus()[2]
    s = orders(stream, 9)["sorted"]
    path = bam_file(tmp_path / "in.bam", header, contigs, s)
    want = post(path, markdup=True, collate=True, coverage=io.StringIO())
    for bb in BATCHES:
        for w in WINDOWS:
            got = post(path, markdup=True, collate=True, coverage=io.StringIO(), batch_bytes=bb, sort_window=w)
            ref = post(path, markdup=True, collate=True, coverage=io.StringIO(), sort_window=w)
            assert got[0] == ref[0] and got[1] == ref[1] and got[2]["markdup"] == want[2]["markdup"], (bb, w)
            assert BamFile(got[0]).stream == BamFile(want[0]).stream, (bb, w)
            assert all(np.array_equal(got[2]["coverage"][k], v) for k, v in want[2]["coverage"].items()), (bb, w)
            assert bb is None or got[2]["counts"]["batches"] > 1
    spilled = post(path, markdup=True, collate=True, coverage=io.StringIO(), batch_bytes=4096, sort_mem=1)
    assert spilled[0] == want[0] and spilled[1] == want[1] and spilled[2]["markdup"] == want[2]["markdup"]


def test_sam_text_input(tmp_path):
    """the SAM text of a golden set with its lines in coordinate order gives the file of the BAM with the same records"""
    what, contigs, header, stream, body = sorted(golden_all(), key=lambda g: -len(g[3]))[0]
    lines = body.splitlines(True)
    recs = split_records(stream)
    assert len(lines) == len(recs)
    order = sorted(range(len(recs)), key=lambda i: ((fields(recs[i])[0] & 0xFFFFFFFF), fields(recs[i])[1], i))
    sam = tmp_path / "s.sam"
    sam.write_bytes(header.encode() + b"".join(lines[i] for i in order))
    bam = bam_file(tmp_path / "s.bam", header, contigs, b"".join(recs[i] for i in order))
    a, b = post(str(sam), markdup=True, collate=True), post(bam, markdup=True, collate=True)
    assert a[0] == b[0] and a[1] == b[1] and a[2]["markdup"] == b[2]["markdup"]


def test_the_tools_own_output_fed_back(tmp_path):
    what, contigs, header, stream = permuted_corpus()[2]
    first = post(bam_file(tmp_path / "g.bam", header, contigs, stream), markdup=True)
    out = tmp_path / "marked.bam"
    out.write_bytes(first[0])
    again = post(str(out), markdup=True, collate=True)
    assert {c: again[2]["markdup"][c] for c in FOUR} == {c: first[2]["markdup"][c] for c in FOUR}
    assert first[2]["markdup"]["duplicate_pairs"] > 0 and again[2]["counts"]["duplicate_flags_cleared"] == first[2]["markdup"]["records_flagged"]
    f = BamFile(again[0])
    check_file(again[0], again[1], model_header(header), contigs, f.stream, "fed back", n_regions=5)
    assert BamFile(first[0]).stream == f.stream, "equal first records' order: the same duplicates"


# ---------------------------------------------------------------------------------------------------------------- refusals

def refused(tmp_path, stream, match, header=HEADER, host=True, **kw):
    from bwamem_hip.bam import bam_post_file
    path = bam_file(tmp_path / "bad.bam", header, CONTIGS, stream)
    for bb in (None, 1):
        out = io.BytesIO()
        with pytest.raises(ValueError, match=match):
            bam_post_file(path, out, host=host, markdup=True, collate=True, batch_bytes=bb, **kw)
        assert out.getvalue() == b"", "a refusal before the first byte leaves nothing"


def refusal_cases():
    z1, z2 = pair(b"z", 1, 5, False, 1, 50, True), pair(b"z", 1, 700, False, 1, 900, True)
    p = pair(b"p", 1, 100, False, 1, 300, True)
    rg_header = HEADER + "@RG\tID:a\tLB:one\n"
    norg = [tagged(r, b"RGZa\0") for r in filler(0)] + [tagged(z1[0], b"RGZa\0")] + [rec(b"norg", 1, 77, 0)] + [tagged(z1[0], b"RGZa\0")]
    return dict(
        two_whole_pairs=(b"".join(filler(0) + z1 + filler(1) + z2), r"the 4 records of the whole file under the read name of record 3 hold 4 primary lines \(2 with 0x40, 2 with 0x80; paired\)", {}),
        no_read_2=(b"".join(filler(0) + [p[0]] + filler(1)), r"the 1 records of the whole file under the read name of record 3 hold 1 primary lines \(1 with 0x40, 0 with 0x80; paired\)", {}),
        read_1_twice=(b"".join([p[0]] + filler(0) + [p[0], p[1]]), r"the 3 records of the whole file under the read name of record 0 hold 3 primary lines \(2 with 0x40, 1 with 0x80; paired\)", {}),
        two_unpaired=(b"".join([rec(b"u", 1, 5, 0)] + filler(0) + [rec(b"u", 1, 9, 0)]), r"under the read name of record 0 hold 2 primary lines \(0 with 0x40, 0 with 0x80; unpaired\)", {}),
        improper_before_no_rg=(b"".join(norg), r"the 2 records of the whole file under the read name of record 3 hold 2 primary lines", dict(libraries=True, header=rg_header)),
    )


@pytest.mark.parametrize("which", sorted(refusal_cases()))
def test_refusals(tmp_path, which):
    stream, match, kw = refusal_cases()[which]
    refused(tmp_path, stream, match, **kw)
    recs = split_records(stream)
    if "libraries" not in kw:
        with pytest.raises(Refused) as e:
            model_entries(recs)
        assert f"record {e.value.args[0]} hold {e.value.args[1]} primary lines ({e.value.args[2]} with 0x40, {e.value.args[3]} with 0x80" in match.replace("\\", "")


def test_no_read_group_alone_is_refused_by_its_own_index(tmp_path):
    """the same file without the improper set: the first record without RG:Z is what is left to refuse"""
    rg_header = HEADER + "@RG\tID:a\tLB:one\n"
    stream = b"".join([tagged(r, b"RGZa\0") for r in filler(0)] + [rec(b"norg", 1, 77, 0)])
    refused(tmp_path, stream, r"record 3", header=rg_header, libraries=True)


def test_sam_refusal_names_the_line(tmp_path):
    from bwamem_hip.bam import bam_post_file
    line = "%s\t%d\tchr2\t%d\t60\t10M\t=\t%d\t0\tACGTACGTAC\tIIIIIIIIII\n"
    sam = tmp_path / "bad.sam"
    sam.write_text(HEADER + line % ("a", 0x41, 5, 90) + (line % ("b", 0, 7, 0)).replace("=", "*") + line % ("a", 0x41, 90, 5))
    with pytest.raises(ValueError, match=rf"under the read name of record 0 \(line {HEADER.count(chr(10)) + 1}\) hold 2 primary lines \(2 with 0x40, 0 with 0x80; paired\)"):
        bam_post_file(str(sam), io.BytesIO(), host=True, markdup=True, collate=True)


def test_collate_needs_markdup(tmp_path, capsys):
    from bwamem_hip.bam import bam_post_file, main
    path = bam_file(tmp_path / "in.bam", HEADER, CONTIGS, rec(b"a", 1, 5, 0))
    out = io.BytesIO()
    with pytest.raises(ValueError, match="collate needs marking"):
        bam_post_file(path, out, host=True, collate=True)
    with pytest.raises(ValueError, match="collate needs marking"):
        bam_post_file(str(tmp_path / "not there.bam"), out, host=True, collate=True)            # (refused before anything is read)
    assert out.getvalue() == b""
    assert main(["--host", "--collate", path]) == 2 and "--collate needs --markdup" in capsys.readouterr().err
    o = str(tmp_path / "o.bam")
    assert main(["--host", "--markdup", "--collate", "-o", o, path]) == 0 and os.path.getsize(o + ".bai") > 8


def test_forced_collisions_are_refused_never_merged():
    from bwamem_hip.lib import bam_templates
    stream = b"".join(r for i in range(40) for r in pair(b"n%d" % i, 1, 100 + i, False, 1, 400 + i, True))
    whole = bam_templates(stream, host=True)
    assert whole["counts"]["templates"] == 40 and whole["tpl"].tolist() == [i // 2 for i in range(80)]
    for bits in (1, 3):                                        # 40 names on 2 or 8 keys: some two distinct proper templates share one
        with pytest.raises(ValueError, match=r"hold \d+ primary lines"):
            bam_templates(stream, host=True, hash_bits=bits)
    assert bam_templates(stream, host=True, hash_bits=127)["tpl"].tolist() == whole["tpl"].tolist()
    assert bam_templates(stream, host=True, hash_bits=64)["tpl"].tolist() == whole["tpl"].tolist()
    with pytest.raises(ValueError, match="hash_bits"):
        bam_templates(stream, host=True, hash_bits=0)


# ---------------------------------------------------------------------------------------------------------------- the core under the sanitizers

def _build():
    out = os.path.join(HERE, "_build"); os.makedirs(out, exist_ok=True)
    exe = os.path.join(out, "bam_tpl_core_host")
    csrc = os.path.join(HERE, "..", "bwa-mem_gpu_amd", "csrc")
    src = [os.path.join(HERE, "bam_tpl_core_host.cpp")] + [os.path.join(csrc, f) for f in ("bam_tpl_core.h", "bam_post_core.h", "bam_dup_core.h", "bam_cov_core.h", "bam_sort_core.h")]
    if not os.path.exists(exe) or any(os.path.getmtime(s) > os.path.getmtime(exe) for s in src):
        subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", src[0], "-o", exe])
    return exe


def core_cases():
    """(stream, hash_bits): the case table, the first-record case, the refusals and a stream under forged equal keys"""
    cases = [(b"".join(records), 128) for _w, records, _f in table()]
    cases += [(first_record_cases()[0], 128)]
    cases += [(stream, 128) for stream, _m, kw in refusal_cases().values() if "libraries" not in kw]
    cases += [(cases[0][0], 2), (synthetic(60, 3), 128), (synthetic(60, 3), 4)]
    return cases


def test_core_under_sanitizers(tmp_path):
    cases = core_cases()
    fi, fo = str(tmp_path / "tpl_case.bin"), str(tmp_path / "tpl_result.bin")
    with open(fi, "wb") as f:
        f.write(struct.pack("<I", len(cases)) + b"".join(struct.pack("<IQ", bits, len(s)) + s for s, bits in cases))
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0")
    r = subprocess.run([_build(), fi, fo], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    err = r.stderr.decode(errors="replace")
    assert r.returncode == 0 and "Sanitizer" not in err and "runtime error" not in err, "the sanitizers (or the driver) reported:\n" + err[-4000:]
    res, p = open(fo, "rb").read(), 0
    n_refused = 0
    for stream, bits in cases:
        recs = split_records(stream)
        n, word = struct.unpack_from("<IQ", res, p); p += 12
        assert n == len(recs)
        if bits == 128:
            try:
                tpl, entries = model_entries(recs)
                assert word == ONES, "the model takes what the core refuses"
            except Refused as e:
                assert word == e.args[0] << 3 | 1
        if word != ONES:
            n_refused += 1
            continue
        nt = struct.unpack_from("<I", res, p)[0]; p += 4
        got_tpl = list(struct.unpack_from("<%dI" % n, res, p)); p += 4 * n
        got_e = [struct.unpack_from("<QQII", res, p + 24 * t) for t in range(nt)]; p += 24 * nt
        if bits == 128:
            assert got_tpl == tpl and got_e == entries
    assert p == len(res) and n_refused >= 5
