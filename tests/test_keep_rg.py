"""A BAM realigned under its own read groups, the host forms: the header's @RG lines (bam_read_groups), the read group of a read (bam_to_reads(host=True,
read_groups=ids): csrc/bam_in_core.h bi_read_group through csrc/reads_io.cpp), that core function as a stand-alone program under AddressSanitizer and UBSan
(tests/bam_rg_core_host.cpp), and the host formatter with a read group per read (bmh_format_sam_groups) against its own per -R texts picked read by read.

The records are written here with test_bam_input.py's encoder; the expected group of a read is the one its record was given.  GROUP_CASES, REFUSALS and the
mixed tables are shared with test_keep_rg_gpu.py, where the kernels must equal these forms."""
import functools
import os
import struct
import subprocess

import numpy as np
import pytest

import sam_table
from bwamem_hip.aligner import bam_read_groups, bam_to_reads
from test_bam_input import stored, tag

HERE = os.path.dirname(os.path.abspath(__file__))
IDS3 = ["a", "ab", "lane.3-of_three"]                     # `a` is a prefix of `ab`: IDs are compared whole


def rg(i) -> bytes:
    return tag(b"RG", b"Z", i if isinstance(i, bytes) else i.encode())


# one tag of every type, a B array of every element type (an empty one among them): the walk must step over each by its own extent
OTHER_TAGS = [tag(b"a1", b"A", b"q"), tag(b"c1", b"c", -128), tag(b"C1", b"C", 255), tag(b"s1", b"s", -32768), tag(b"S1", b"S", 65535), tag(b"i1", b"i", -2147483648),
              tag(b"I1", b"I", 4294967295), tag(b"f1", b"f", 1.5), tag(b"z1", b"Z", b"RG:Z:ab inside a value"), tag(b"h1", b"H", b"1AE301"), tag(b"z2", b"Z", b""),
              tag(b"bc", b"B", (b"c", [1, -2, 3])), tag(b"bC", b"B", (b"C", [82, 71, 90])), tag(b"bs", b"B", (b"s", [-3])), tag(b"bS", b"B", (b"S", [])),
              tag(b"bi", b"B", (b"i", [7, 8])), tag(b"bI", b"B", (b"I", [0x5a47520a])), tag(b"bf", b"B", (b"f", [0.5, 2.0]))]


# ---------------------------------------------------------------------------------------------------------------- the header's @RG lines

HEADER_OK = {
    "one": (b"@HD\tVN:1.6\n@RG\tID:x\tLB:l1\n@SQ\tSN:c\tLN:9\n", [("@RG\tID:x\tLB:l1", "x", "l1")]),
    "three among other lines": (b"@HD\tVN:1.6\tSO:unsorted\n@RG\tID:a\tLB:l1\tSM:s\n@SQ\tSN:c\tLN:9\n@RG\tID:ab\tSM:s\n@PG\tID:p\n@RG\tID:c\tPL:X\tLB:l1\n@CO\t@RG\tID:no\n",
                                [("@RG\tID:a\tLB:l1\tSM:s", "a", "l1"), ("@RG\tID:ab\tSM:s", "ab", "Unknown Library"), ("@RG\tID:c\tPL:X\tLB:l1", "c", "l1")]),
    "last line without newline": (b"@SQ\tSN:c\tLN:9\n@RG\tID:a\n@RG\tID:b\tLB:z", [("@RG\tID:a", "a", "Unknown Library"), ("@RG\tID:b\tLB:z", "b", "z")]),
    "CR LF": (b"@HD\tVN:1.6\r\n@RG\tID:a\tLB:z\r\n@RG\tID:b\r\n", [("@RG\tID:a\tLB:z", "a", "z"), ("@RG\tID:b", "b", "Unknown Library")]),
    "NUL padding": (b"@RG\tID:a\n\0\0\0@RG\tID:behind\n", [("@RG\tID:a", "a", "Unknown Library")]),
    "an ID of 1 byte and of 255": (b"@RG\tID:q\n@RG\tID:" + b"q" * 255 + b"\n", [("@RG\tID:q", "q", "Unknown Library"), ("@RG\tID:" + "q" * 255, "q" * 255, "Unknown Library")]),
}
HEADER_BAD = {
    "zero": (b"@HD\tVN:1.6\n@SQ\tSN:c\tLN:9\n@CO\t@RG\tID:a\n", "no @RG line"),
    "empty text": (b"", "no @RG line"),
    "an ID of 256 bytes": (b"@RG\tID:a\n@RG\tID:" + b"q" * 256 + b"\n", r"@RG line 2 .*longer than 255"),
    "a repeated ID": (b"@RG\tID:a\tLB:x\n@RG\tID:b\n@RG\tID:a\tLB:y\n", r"@RG line 3 .*earlier @RG line"),
    "without ID": (b"@RG\tID:a\n@RG\tLB:x\tSM:s\n", r"@RG line 2 .*no ID"),
    "an empty ID": (b"@RG\tID:\tLB:x\n", r"@RG line 1 .*no ID"),
    "a field that is no XX:value": (b"@RG\tID:a\tLBx\n", r"@RG line 1 .*not XX:value"),
    "blanks for tabs": (b"@RG ID:a\n@RG\tID:b SM:s\tx\n", r"@RG line 1 .*not XX:value"),
}


@pytest.mark.parametrize("case", list(HEADER_OK))
def test_header_lines(case):
    text, want = HEADER_OK[case]
    assert bam_read_groups(text) == want and bam_read_groups(text, markdup=True) == want and bam_read_groups(text.decode()) == want


@pytest.mark.parametrize("case", list(HEADER_BAD))
def test_header_refusals(case):
    text, msg = HEADER_BAD[case]
    with pytest.raises(ValueError, match=msg):
        bam_read_groups(text)


def test_header_256_libraries_only_refused_with_markdup():
    text = "".join("@RG\tID:g%d\tLB:lib%d\n" % (k, k) for k in range(256))
    got = bam_read_groups(text)
    assert len(got) == 256 and [g[2] for g in got] == ["lib%d" % k for k in range(256)]
    with pytest.raises(ValueError, match=r"@RG line 256 .*256th"):
        bam_read_groups(text, markdup=True)
    one_less = "".join("@RG\tID:g%d\tLB:lib%d\n" % (k, k % 255) for k in range(300))        # 300 groups in 255 libraries
    assert len(bam_read_groups(one_less, markdup=True)) == 300


# ---------------------------------------------------------------------------------------------------------------- a read's group

def _rec(k, gid, flag=4, tags_before=b"", tags_after=b"", L=None, rev=False):
    L = L or 5 + k % 7
    seq = bytes(b"ACGT"[(k + i * (1 + k % 3)) & 3] for i in range(L))
    return stored(b"r%d" % k, seq, bytes(40 + (i + k) % 30 for i in range(L)), flag, tags_before + (rg(gid) if gid is not None else b"") + tags_after, rev=rev)


@functools.lru_cache(maxsize=None)
def group_cases() -> dict:
    """name -> (records, the IDs of the table, the expected group of every read)"""
    out = {}
    # the tag first, last, and between the tags of every type
    recs, want = [], []
    n_t = len(OTHER_TAGS)
    for k in range(n_t + 1):
        g = k % 3
        recs.append(_rec(k, IDS3[g], tags_before=b"".join(OTHER_TAGS[:k]), tags_after=b"".join(OTHER_TAGS[k:])))
        want.append(g)
    recs.append(_rec(n_t + 1, "ab")); want.append(1)                               # the only tag
    recs.append(_rec(n_t + 2, "a", tags_after=rg("ab"))); want.append(0)           # the first RG tag decides
    out["the tag at every place"] = (b"".join(recs), IDS3, want)
    out["a and ab, either order of the table"] = (b"".join(_rec(k, ("a", "ab")[k & 1]) for k in range(9)), ["ab", "a"], [1 - (k & 1) for k in range(9)])
    # skipped records carry no tag, another type's tag or an unknown ID: they are never inspected
    recs, want = [], []
    for k in range(30):
        recs.append(_rec(k, IDS3[k % 3], rev=k % 5 == 0)); want.append(k % 3)
        if k % 4 == 1:
            recs.append(_rec(100 + k, None, flag=0x100))
        if k % 4 == 2:
            recs.append(_rec(100 + k, "nowhere", flag=0x800 | 0x10))
        if k % 4 == 3:
            recs.append(stored(b"s%d" % k, b"ACG", b"III", 0x900, tag(b"RG", b"i", 7)))
    out["skipped records are not inspected"] = (b"".join(recs), IDS3, want)
    # pairs: both records of one group, in either order in the file; the read order is 0x40 then 0x80
    recs, want = [], []
    for k in range(12):
        a = stored(b"p%d" % k, b"ACGTA", b"IIIII", 0x4d, rg(IDS3[k % 3]))
        b = stored(b"p%d" % k, b"TTGCA", b"JJJJJ", 0x8d, tag(b"XY", b"i", k) + rg(IDS3[k % 3]), rev=bool(k & 1))
        recs += [b, a] if k % 4 == 2 else [a, b]
        if k % 5 == 0:
            recs.append(stored(b"p%d" % k, b"AC", b"II", 0x900 | 0x41))
        want += [k % 3, k % 3]
    out["pairs"] = (b"".join(recs), IDS3, want)
    return out


@pytest.mark.parametrize("case", list(group_cases()))
def test_host_groups(case):
    records, ids, want = group_cases()[case]
    rs = bam_to_reads(records, host=True, read_groups=ids)
    assert rs.groups.dtype == np.uint32 and rs.groups.tolist() == want
    plain = bam_to_reads(records, host=True)                     # nothing else about the reads changes, with or without comments
    assert plain.groups is None
    for a, b in ((rs, plain), (bam_to_reads(records, comments=True, host=True, read_groups=ids), bam_to_reads(records, comments=True, host=True))):
        assert np.array_equal(a.ascii, b.ascii) and np.array_equal(a.lens, b.lens) and np.array_equal(a.name_blob, b.name_blob) and np.array_equal(a.qual, b.qual)
        assert (a.comments is None) == (b.comments is None) and (a.comments is None or np.array_equal(a.comments[0], b.comments[0]))
    assert b"RG:Z" not in bam_to_reads(records, comments=True, host=True, read_groups=ids).comments[0].tobytes().replace(b"z1:Z:RG:Z:ab inside a value", b"")


@functools.lru_cache(maxsize=None)
def refusals() -> dict:
    """name -> (records, IDs, a piece of the message, the index of the record it names)"""
    good = [_rec(k, IDS3[k % 3]) for k in range(6)]
    skipped = _rec(50, None, flag=0x100)
    out = {
        "no RG tag": (b"".join(good[:3] + [skipped, _rec(7, None, tags_before=OTHER_TAGS[0] + OTHER_TAGS[11])] + good[3:]), IDS3, "no RG tag", 4),
        "RG:i": (b"".join(good[:2] + [stored(b"bad", b"ACG", b"III", 4, OTHER_TAGS[8] + tag(b"RG", b"i", 1) + rg("a"))] + good[2:]), IDS3, "RG tag of a type other than Z", 2),
        "an unknown ID": (b"".join([skipped] + good + [_rec(8, "abc")]), IDS3, "read group the header's @RG lines do not hold", 7),
        "a prefix of an ID": (b"".join(good + [_rec(8, "lane.3")]), IDS3, "read group the header's @RG lines do not hold", 6),
        "an empty ID": (b"".join([_rec(8, "")] + good), IDS3, "read group the header's @RG lines do not hold", 0),
    }
    pair = lambda k, g1, g2: [stored(b"p%d" % k, b"ACGTA", b"IIIII", 0x4d, rg(g1)), stored(b"p%d" % k, b"TTGCA", b"JJJJJ", 0x8d, rg(g2))]
    out["a pair of two groups"] = (b"".join(pair(0, "a", "a") + [stored(b"p0", b"AC", b"II", 0x941)] + pair(1, "ab", "ab") + pair(2, "a", "ab") + pair(3, "a", "a")), IDS3, "name different read groups (a and ab)", 5)
    out["the second record of a pair without a tag"] = (b"".join(pair(0, "a", "a") + [stored(b"p1", b"ACGTA", b"IIIII", 0x4d, rg("a")), stored(b"p1", b"TTGCA", b"JJJJJ", 0x8d)]), IDS3, "no RG tag", 3)
    return out


@pytest.mark.parametrize("case", list(refusals()))
def test_host_refusals(case):
    records, ids, piece, index = refusals()[case]
    with pytest.raises(ValueError) as e:
        bam_to_reads(records, host=True, read_groups=ids)
    msg = str(e.value)
    assert piece in msg and (f"record {index} " in msg or f"records {index} and {index + 1} " in msg), msg
    assert len(bam_to_reads(records, host=True)) > 0                             # (without a table the same records are reads)


def test_table_refusals():
    rec = _rec(0, "a")
    for ids, msg in (([], "0 read groups"), (["a", "b", "a"], "share the ID"), (["a", ""], "0 bytes"), (["q" * 256], "256 bytes")):
        with pytest.raises(ValueError, match=msg):
            bam_to_reads(rec, host=True, read_groups=ids)
    assert bam_to_reads(rec, host=True, read_groups=["q" * 255, "a"]).groups.tolist() == [1]


# ---------------------------------------------------------------------------------------------------------------- the core under the sanitizers

@pytest.fixture(scope="module")
def rg_core_exe():
    out = os.path.join(HERE, "_build"); os.makedirs(out, exist_ok=True)
    exe = os.path.join(out, "bam_rg_core_host")
    src = [os.path.join(HERE, "bam_rg_core_host.cpp"), os.path.join(HERE, "..", "bwa-mem_gpu_amd", "csrc", "bam_in_core.h")]
    if not os.path.exists(exe) or any(os.path.getmtime(s) > os.path.getmtime(exe) for s in src):
        subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", src[0], "-o", exe])
    return exe


def split_records(data: bytes) -> list:
    out, p = [], 0
    while len(data) - p >= 4:
        e = p + 4 + struct.unpack_from("<I", data, p)[0]
        out.append(data[p:e]); p = e
    return out


def test_core_under_sanitizers(rg_core_exe, tmp_path):
    """every record of the cases gives its group, every refused one its status (8 no tag, 9 another type, 10 unknown), a record cut inside its RG tag is
    bi_check's to refuse -- and no byte outside a record, the IDs or the offsets is read"""
    recs, want = [], []
    for name, (records, ids, groups) in group_cases().items():
        if ids != IDS3:
            continue
        it = iter(groups)
        for r in split_records(records):
            fl = struct.unpack_from("<H", r, 18)[0]
            if fl & 0x900:
                continue
            recs.append(r); want.append((0, 0, next(it)))
    for name, (records, _ids, piece, index) in refusals().items():
        if "pair" in name:
            continue
        r = split_records(records)[index]
        recs.append(r); want.append((0, 8 if "no RG tag" in piece else 9 if "other than Z" in piece else 10, 0))
    last = _rec(3, IDS3[2])                                       # the RG tag is the record's last bytes: the compare ends with the record
    recs.append(last); want.append((0, 0, 2))
    cut = last[:-3]                                               # ... and cut inside the value: the tag runs past the end
    recs.append(struct.pack("<I", len(cut) - 4) + cut[4:]); want.append((4,))
    cases, res = tmp_path / "cases.bin", tmp_path / "res.bin"
    with open(cases, "wb") as f:
        f.write(struct.pack("<I", len(IDS3)) + b"".join(struct.pack("<I", len(i)) + i.encode() for i in IDS3))
        f.write(struct.pack("<I", len(recs)) + b"".join(struct.pack("<I", len(r)) + r for r in recs))
    subprocess.check_call([rg_core_exe, str(cases), str(res)])
    got, data, p = [], open(res, "rb").read(), 0
    for w in want:
        n = 1 if w[0] else 3
        got.append(struct.unpack_from("<%di" % n, data, p)); p += 4 * n
    assert p == len(data) and got == want and len(want) >= 60


# ---------------------------------------------------------------------------------------------------------------- the host formatter, a read group per read

def mixed_tables():
    """(table, options, with qualities and comments, the group index of every read): single-end reads that alternate between three groups -- unmapped, secondary,
    supplementary and XA records among them -- and pairs whose two reads share a group"""
    se = sam_table.Table(sam_table.SE)
    pe = sam_table.Table(sam_table.PE, paired=True)
    return [(se, dict(copy_comment=1), True, [r % 3 for r in range(se.n)]), (pe, {}, False, [(r // 2) % 3 for r in range(pe.n)])]


def host_text(T, po, tags, read_groups=None) -> bytes:
    from bwamem_hip.lib import format_sam
    nb, no = T.blob(T.names)
    cb, co = T.blob(T.comments)
    return format_sam(po, (nb, no[:-1]), T.codes, T.offs, T.lens, T.contigs, T.fin, T.fpr, T.slot, T.aln.reshape(-1, 8), T.cigar, T.md, h_rec=T.h_rec if T.paired else None,
                      unflag=T.unflag if T.paired else None, as_bytes=True, quals=T.quals if tags else None, comments=(cb, co[:-1]) if tags else None, read_groups=read_groups)


def picked(T, opts, tags, groups) -> bytes:
    """the per -R texts of the table picked read by read: every read's lines from the text under its own group's ID"""
    per = []
    for i in IDS3:
        by = {}
        for line in host_text(T, sam_table.post_opt(dict(opts, rg_id=i.encode())), tags).split(b"\n")[:-1]:
            by.setdefault(line.split(b"\t")[0], []).append(line)
        per.append(by)
    out, seen = [], set()
    for r, name in enumerate(T.names):
        if name in seen:                                          # (a pair's second read: its lines came with the first's, in the text's order)
            continue
        seen.add(name)
        out += per[groups[r]][name.encode()]
    return b"".join(l + b"\n" for l in out)


def test_host_formatter_per_read_groups():
    for T, opts, tags, groups in mixed_tables():
        want = picked(T, opts, tags, groups)
        got = host_text(T, sam_table.post_opt(opts), tags, read_groups=(IDS3, groups))
        assert got == want and all(got.count(b"\tRG:Z:" + i.encode() + b"\t") + got.count(b"\tRG:Z:" + i.encode() + b"\n") >= 2 for i in IDS3)
        assert got.count(b"\tRG:Z:") == got.count(b"\n")
        with pytest.raises(RuntimeError, match="beside the options' one read group"):
            host_text(T, sam_table.post_opt(dict(opts, rg_id=b"x")), tags, read_groups=(IDS3, groups))
        with pytest.raises(RuntimeError, match="the table holds 3"):
            host_text(T, sam_table.post_opt(opts), tags, read_groups=(IDS3, [3] + groups[1:]))
