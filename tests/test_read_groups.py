"""Runs over several read groups, host side: duplicates per library (csrc/bam_dup_core.h's library rule, csrc/bam_dup_host.cpp) against test_bam_dup's model
applied library by library, the new core code under AddressSanitizer and UBSan (tests/bam_dup_groups_host.cpp), the header and -R parsing, the per-library metrics
and the refusals of the command and of align_groups.  The same corpus runs on the device in test_read_groups_gpu.py.

The oracle: split the stream's templates by library (that of the RG:Z tag on a template's first record) keeping their order, run `model` on every sub-stream, put
the records back where they were.  Templates keep their relative order inside a library, so the ordinal tie-break of the sub-stream is that of the whole run."""
import io
import os
import struct
import subprocess

import numpy as np
import pytest

from test_bam_dup import DUP, flag_of, mask_dup, model, name_of, one_key, pair, rec, synthetic, table_stream, templates_of
from test_bam_sort import CONTIGS, BamFile, check_file, split_records

HERE = os.path.dirname(os.path.abspath(__file__))
HDR = "@HD\tVN:1.6\tSO:coordinate\n@SQ\tSN:x\tLN:1\n"
# three read groups of which two are lanes of one library
GROUPS = [("lane1", "libA"), ("lane2", "libB"), ("lane3", "libA")]
COUNT_KEYS = ("pairs_examined", "fragments_examined", "duplicate_pairs", "duplicate_fragments", "records_flagged", "secondary_or_supplementary", "unmapped_records", "templates")


# ---------------------------------------------------------------------------------------------------------------- tagged streams

def tag(r: bytes, rid: str) -> bytes:
    """the record with RG:Z:<rid> appended and block_size fixed"""
    r = r + b"RGZ" + rid.encode() + b"\0"
    return struct.pack("<I", len(r) - 4) + r[4:]


def tagged(stream: bytes, id_of_template) -> bytes:
    """every record of template t tagged with id_of_template(t, name of its first record)"""
    recs = split_records(stream)
    out = list(recs)
    for t, idx in enumerate(templates_of(recs)):
        rid = id_of_template(t, name_of(recs[idx[0]]))
        for i in idx:
            out[i] = tag(recs[i], rid)
    return b"".join(out)


def rg_of(r: bytes):
    """the RG:Z value by a walk over the record's tags (None: none)"""
    l_name, n_ops, l_seq = r[12], struct.unpack_from("<H", r, 16)[0], struct.unpack_from("<I", r, 20)[0]
    p = 36 + l_name + 4 * n_ops + (l_seq + 1) // 2 + l_seq
    width = {"A": 1, "c": 1, "C": 1, "s": 2, "S": 2, "i": 4, "I": 4, "f": 4}
    while p + 3 <= len(r):
        t, ty = r[p:p + 2], chr(r[p + 2]); p += 3
        if ty in "ZH":
            e = r.index(b"\0", p)
            if t == b"RG" and ty == "Z":
                return r[p:e].decode()
            p = e + 1
        elif ty == "B":
            p += 5 + width[chr(r[p])] * struct.unpack_from("<I", r, p + 1)[0]
        else:
            p += width[ty]
    return None


def library_model(stream: bytes, groups):
    """(the records flagged per library, the total counts, {library: counts}, {library: what it holds}) -- `model` on every library's templates"""
    lib_of = dict(groups)
    recs = split_records(stream)
    tpls = templates_of(recs)
    libs = list(dict.fromkeys(lb for _id, lb in groups))
    members = {lb: [] for lb in libs}
    for idx in tpls:
        members[lib_of[rg_of(recs[idx[0]])]].append(idx)
    out = list(recs)
    per, holds = {}, {}
    for lb in libs:
        flat = [i for idx in members[lb] for i in idx]
        marked, counts, h = model(b"".join(recs[i] for i in flat))
        for i, r in zip(flat, split_records(marked)):
            out[i] = r
        per[lb], holds[lb] = counts, h
    total = {k: sum(per[lb][k] for lb in libs) for k in COUNT_KEYS}
    return b"".join(out), total, per, holds


def round_robin(t, _name):
    return GROUPS[t % 3][0]


def one_key_two_libraries() -> bytes:
    """test_bam_dup.one_key's 300 pairs at one key alternate between libA and libB; its fragment at the pairs' end is of libC, which has no pair there; one more
    fragment at that end is of libA; the fragment elsewhere is of libA"""
    s = one_key(300) + rec(b"fr_at_end_libA", 1, 700, 0, q=40)

    def ids(t, name):
        if name == b"fr_at_end":
            return "c"
        if name.startswith(b"p"):
            return "a" if int(name[1:]) % 2 == 0 else "b"
        return "a"
    return tagged(s, ids)


ONE_KEY_GROUPS = [("a", "libA"), ("b", "libB"), ("c", "libC")]
_CORPUS = []


def corpus():
    """(what, groups, stream, must): must = what every library of the member has to hold by the oracle"""
    if not _CORPUS:
        every = {"pair", "frag", "clean"}
        for n in (0, 1, 63, 64, 65, 257, 1000):
            _CORPUS.append(("synthetic %d" % n, GROUPS, tagged(synthetic(n, 100 + n), round_robin), every if n >= 257 else set()))
        _CORPUS.append(("300 pairs at one key, two libraries", ONE_KEY_GROUPS, one_key_two_libraries(), set()))
        _CORPUS.append(("table, one group", [("only", "lib")], tagged(table_stream(), lambda t, n: "only"), every))
    return _CORPUS


_ORACLE = {}


def expected(what, groups, stream):
    if what not in _ORACLE:
        _ORACLE[what] = library_model(stream, groups)
    return _ORACLE[what]


def pair_key(recs, idx):
    """(library-free) key of a template when it is a pair with both lines mapped, else None"""
    from test_bam_dup import end_word
    pri = [recs[i] for i in idx if not flag_of(recs[i]) & 0x900]
    if len(pri) == 2 and not any(flag_of(p) & 4 for p in pri):
        return tuple(sorted(end_word(p) for p in pri))
    return None


# ---------------------------------------------------------------------------------------------------------------- the rule

def test_corpus_is_not_vacuous():
    for what, groups, stream, must in corpus():
        _m, _t, per, holds = expected(what, groups, stream)
        for lb in per:
            assert must <= holds[lb], (what, lb, holds[lb], per[lb])
    # a key that occurs in two libraries, with a pair that stays in each: no duplicate is called across them
    what, groups, stream, _must = corpus()[6]
    marked = split_records(expected(what, groups, stream)[0])
    lib_of = dict(groups)
    kept = {}
    for idx in templates_of(marked):
        k = pair_key(marked, idx)
        if k is not None and not flag_of(marked[idx[0]]) & DUP:
            kept.setdefault(k, set()).add(lib_of[rg_of(marked[idx[0]])])
    assert any(len(v) == 2 for v in kept.values())
    # ... and the whole-stream model does call duplicates across them: the libraries change the answer
    assert model(stream)[0] != expected(what, groups, stream)[0]


def test_one_key_in_two_libraries():
    what, groups, stream, _must = corpus()[7]
    marked, total, per, _h = expected(what, groups, stream)
    recs = split_records(marked)
    by_name = {name_of(r): flag_of(r) & DUP for r in recs}
    for lb, parity in (("libA", 0), ("libB", 1)):
        kept = [n for n, d in by_name.items() if n.startswith(b"p") and int(n[1:]) % 2 == parity and not d]
        assert len(kept) == 1 and per[lb]["pairs_examined"] == 150 and per[lb]["duplicate_pairs"] == 149, (lb, kept)
    assert by_name[b"fr_at_end_libA"] and not by_name[b"fr_at_end"] and not by_name[b"fr_alone"]      # a pair's end makes a duplicate in its own library only
    assert per["libC"]["fragments_examined"] == 1 and per["libC"]["duplicate_fragments"] == 0 and per["libA"]["duplicate_fragments"] == 1


def test_host_equals_the_library_model():
    from bwamem_hip.lib import bam_markdup
    for what, groups, stream, _must in corpus():
        want, total, per, _h = expected(what, groups, stream)
        got, c = bam_markdup(stream, host=True, read_groups=groups)
        libs = c.pop("libraries")
        assert got == want, what
        assert c == total and libs == per and list(libs) == list(per), what
        assert mask_dup(got) == stream, what
    # a single group: today's answer
    what, groups, stream, _must = corpus()[8]
    plain, pc = bam_markdup(table_stream(), host=True)
    got, c = bam_markdup(stream, host=True, read_groups=groups)
    assert [flag_of(r) for r in split_records(got)] == [flag_of(r) for r in split_records(plain)] and c["libraries"] == {"lib": pc}


def test_without_a_table_the_tags_are_not_read():
    from bwamem_hip.lib import bam_markdup
    for what, _groups, stream, _must in corpus():
        want, counts, _h = model(stream)
        got, c = bam_markdup(stream, host=True)
        assert got == want and c == counts, what
    # tags that cannot be walked, and IDs no table would hold, change nothing either
    s = tagged(synthetic(65, 9), lambda t, n: "zz%d" % t)
    broken = b"".join(r[:-1] + b"x" for r in split_records(s))             # the RG:Z value loses its terminator
    assert bam_markdup(broken, host=True)[0] == model(broken)[0]


@pytest.mark.parametrize("window", [0, 1, 7, 100])
def test_sorted_file_host(window):
    from bwamem_hip.lib import bam_sorted_file
    for what, groups, stream, _must in corpus():
        want, total, per, _h = expected(what, groups, stream)
        bam, bai, c = bam_sorted_file(HDR, CONTIGS, stream, 1, window, host=True, markdup=True, read_groups=groups)
        assert c.pop("libraries") == per and c == total, what
        f = check_file(bam, bai, HDR, CONTIGS, want, (what, window), n_regions=10)
        plain = BamFile(bam_sorted_file(HDR, CONTIGS, stream, 1, window, host=True)[0])
        assert mask_dup(f.stream) == plain.stream, what


def test_refusals():
    from bwamem_hip.lib import bam_markdup, bam_sorted_file
    s = tagged(synthetic(65, 9), round_robin)
    recs = split_records(s)
    idx = templates_of(recs)[7][0]
    untagged = b"".join(recs[:idx]) + b"".join(split_records(synthetic(65, 9))[idx:idx + 1]) + b"".join(recs[idx + 1:])
    for call in (lambda x, g: bam_markdup(x, host=True, read_groups=g), lambda x, g: bam_sorted_file(HDR, CONTIGS, x, 1, 0, host=True, markdup=True, read_groups=g)):
        with pytest.raises(ValueError, match=r"record %d .*no RG:Z tag" % idx):
            call(untagged, GROUPS)
        with pytest.raises(ValueError, match=r"record 2 .*not among those given"):            # template 1 (records 2 ..) is of lane2
            assert rg_of(recs[2]) == "lane2"
            call(s, [g for g in GROUPS if g[0] != "lane2"])
        with pytest.raises(ValueError, match=r"read group 256 .*at most 255 libraries"):
            call(s, GROUPS + [("x%d" % k, "lib%d" % k) for k in range(254)])
        with pytest.raises(ValueError, match=r"read groups 1 and 3 share the ID 'lane2'"):
            call(s, GROUPS + [("lane2", "libC")])
        with pytest.raises(ValueError, match="no read groups"):
            call(s, [])
    call = lambda x, g: bam_markdup(x, host=True, read_groups=g)
    got, c = call(s, GROUPS + [("x%d" % k, "lib%d" % k) for k in range(253)])                 # 255 libraries are taken
    assert len(c["libraries"]) == 255 and got == expected("synthetic 65 again", GROUPS, s)[0]
    with pytest.raises(ValueError, match="read_groups needs markdup"):
        bam_sorted_file(HDR, CONTIGS, s, 1, 0, host=True, read_groups=GROUPS)
    far = tagged(rec(b"far", 1 << 24, 5, 0), lambda t, n: "lane1")                            # a refID the key has no room for beside the library
    with pytest.raises(ValueError, match=r"record 0 names reference 16777216"):
        bam_markdup(far, host=True, read_groups=GROUPS)
    assert bam_markdup(far, host=True)[1]["fragments_examined"] == 1


# ---------------------------------------------------------------------------------------------------------------- the core under the sanitizers

def _build():
    out = os.path.join(HERE, "_build"); os.makedirs(out, exist_ok=True)
    exe = os.path.join(out, "bam_dup_groups_host")
    csrc = os.path.join(HERE, "..", "bwa-mem_gpu_amd", "csrc")
    src = [os.path.join(HERE, "bam_dup_groups_host.cpp")] + [os.path.join(csrc, f) for f in ("bam_dup_core.h", "bam_dup.h", "bam_dup_host.cpp", "bam_sort_core.h")]
    if not os.path.exists(exe) or any(os.path.getmtime(s) > os.path.getmtime(exe) for s in src):
        subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", src[0], "-o", exe])
    return exe


def run_core(tmp_path, cases):
    """cases: (groups as [(id, library index)], stream) -> [(rc, flags, counts, per-library counts)]"""
    fi, fo = str(tmp_path / "groups_case.bin"), str(tmp_path / "groups_result.bin")
    with open(fi, "wb") as f:
        f.write(struct.pack("<I", len(cases)))
        for groups, s in cases:
            f.write(struct.pack("<I", len(groups)) + b"".join(struct.pack("<B", len(i)) + i + struct.pack("<i", lb) for i, lb in groups) + struct.pack("<Q", len(s)) + s)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0")
    r = subprocess.run([_build(), fi, fo], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    err = r.stderr.decode(errors="replace")
    assert r.returncode == 0 and "Sanitizer" not in err and "runtime error" not in err, "the sanitizers (or the driver) reported:\n" + err[-4000:]
    with open(fo, "rb") as f:
        res = f.read()
    out, p = [], 0
    for _c in cases:
        rc = struct.unpack_from("<i", res, p)[0]; p += 4
        if rc != 0:
            out.append((rc, None, None, None))
            continue
        n = struct.unpack_from("<I", res, p)[0]; p += 4
        flags = struct.unpack_from("<%dH" % n, res, p); p += 2 * n
        counts = struct.unpack_from("<8Q", res, p); p += 64
        nl = struct.unpack_from("<I", res, p)[0]; p += 4
        out.append((0, flags, counts, [struct.unpack_from("<8Q", res, p + 64 * k) for k in range(nl)])); p += 64 * nl
    assert p == len(res)
    return out


def indexed(groups):
    libs = list(dict.fromkeys(lb for _i, lb in groups))
    return [(i.encode(), libs.index(lb)) for i, lb in groups], libs


def test_core_under_sanitizers(tmp_path):
    members = corpus()
    res = run_core(tmp_path, [(indexed(g)[0], s) for _w, g, s, _m in members])
    for (what, groups, stream, _must), (rc, flags, counts, per_lib) in zip(members, res):
        want, total, per, _h = expected(what, groups, stream)
        assert rc == 0 and list(flags) == [flag_of(r) for r in split_records(want)], what
        assert dict(zip(COUNT_KEYS, counts)) == total, what
        assert [dict(zip(COUNT_KEYS, c)) for c in per_lib] == [per[lb] for lb in indexed(groups)[1]], what
    s = members[3][2]
    g = indexed(GROUPS)[0]
    bad = [(g[:1], s), (g + [(b"lane2", 1)], s), (g + [(b"far", 255)], s), ([], s), (g + [(b"", 0)], s), (g, s[:-1]), (g, mask_dup(synthetic(64, 164)))]
    assert [rc for rc, _f, _c, _l in run_core(tmp_path, bad)] == [-2] * len(bad)
    # 2000 damaged streams: bytes of two tagged streams overwritten, cut or repeated -- the tags' types, lengths and terminators among them: refused or marked,
    # never read out of bounds
    rng = np.random.default_rng(5)
    base = [members[8][2], members[2][2]]
    damaged = []
    for k in range(2000):
        b = bytearray(base[k & 1])
        for _ in range(int(rng.integers(1, 6))):
            i = int(rng.integers(0, len(b)))
            b[i] = int(rng.integers(0, 256))
        if k % 3 == 0:                                                     # ... and one aimed at a tag: its type byte, or its terminator
            r0 = 0
            for r in split_records(base[k & 1])[:int(rng.integers(1, 20))]:
                r0 += len(r)
            b[r0 - (1 if k % 6 == 0 else 4 + len("lane1"))] = int(rng.integers(0, 256))
        if k % 5 == 0:
            b = b[:int(rng.integers(0, len(b)))]
        damaged.append(([(b"only", 0)] if not k & 1 else g, bytes(b)))
    res = run_core(tmp_path, damaged)
    assert len(res) == 2000 and all(rc in (0, -2) for rc, _f, _c, _l in res) and any(rc == 0 for rc, _f, _c, _l in res) and any(rc == -2 for rc, _f, _c, _l in res)


# ---------------------------------------------------------------------------------------------------------------- header, -R, metrics, keywords, the command

def test_header_lists_every_read_group_and_R_is_parsed_as_before():
    from bwamem_hip.aligner import Aligner, parse_rg_line
    al = Aligner.__new__(Aligner)
    al.contigs = [("a", 5), ("b", 7)]
    assert Aligner.header(al) == "@SQ\tSN:a\tLN:5\n@SQ\tSN:b\tLN:7\n"
    al._groups = [parse_rg_line(v, "group") + ("r.fa", None) for v in ("@RG\\tID:l2\\tLB:x", "@RG\\tID:l1\\tLB:x\\tSM:s 1", "@RG\\tID:l3")]
    assert Aligner.header(al) == "@SQ\tSN:a\tLN:5\n@SQ\tSN:b\tLN:7\n@RG\tID:l2\tLB:x\n@RG\tID:l1\tLB:x\tSM:s 1\n@RG\tID:l3\n"
    # the cases of test_options.py through the helper, and through set_options as before
    assert parse_rg_line("@RG\\tID:grp.1\\tSM:s 1\\tPL:x") == ("@RG\tID:grp.1\tSM:s 1\tPL:x", "grp.1")
    assert parse_rg_line("@RG\\tID:a\\\\tb\\qc\\nSM:x") == ("@RG\tID:a\\tbc\nSM:x", "a\\tbc")
    for bad in ("RG\\tID:x", "@RG\\tSM:x", "@RG\\tID:" + "x" * 256):
        with pytest.raises(ValueError, match="^--rg: "):
            parse_rg_line(bad, "--rg")
        with pytest.raises(ValueError, match="^-R: "):
            parse_rg_line(bad)

    class _Opts:
        pass
    from bwamem_hip.lib import ChainOpt, ExtParams, PeOpt, PostOpt, ReseedOpt
    o = _Opts()
    o.copt, o.ep, o.po, o.pe, o.reseed = ChainOpt(), ExtParams(), PostOpt(), PeOpt(), ReseedOpt()
    for v in ("@RG\\tID:grp.1\\tSM:s 1\\tPL:x", "@RG\\tID:a\\\\tb\\qc\\nSM:x"):
        Aligner.set_options(o, ["-R", v])
        assert (o.rg_line, o.po.rg_id.decode()) == parse_rg_line(v)


def test_metrics_have_one_row_per_library():
    from bwamem_hip.aligner import markdup_metrics_text, markdup_metrics_text_libraries
    what, groups, stream, _must = corpus()[6]
    _m, total, per, _h = expected(what, groups, stream)
    lines = markdup_metrics_text_libraries(per).split("\n")
    one = markdup_metrics_text(total, "@RG\tID:x\tLB:all").split("\n")
    assert lines[:2] == one[:2] and len(lines) == 5 and lines[4] == ""
    rows = [l.split("\t") for l in lines[2:4]]
    assert [r[0] for r in rows] == ["libA", "libB"]                          # first appearance: lane1 is of libA
    assert [sum(int(r[k]) for r in rows) for k in range(1, 7)] == [int(v) for v in one[2].split("\t")[1:7]]
    for r, lb in zip(rows, ("libA", "libB")):
        assert r == markdup_metrics_text(per[lb], "@RG\tID:x\tLB:" + lb).split("\n")[2].split("\t")


def test_align_groups_keywords():
    from bwamem_hip.aligner import Aligner
    al = Aligner.__new__(Aligner)                                         # the keyword checks come before anything touches an index or a device
    al.profile = False
    two = [("@RG\\tID:a\\tLB:x", "a.fa", None), ("@RG\\tID:b\\tLB:x", "b_1.fq", "b_2.fq")]
    for call in (lambda: al.align_groups(two),                                                          # no out
                 lambda: al.align_groups([], out=io.BytesIO()),
                 lambda: al.align_groups([("RG\\tID:a", "a.fa", None)], out=io.BytesIO()),
                 lambda: al.align_groups([("@RG\\tSM:a", "a.fa", None)], out=io.BytesIO()),
                 lambda: al.align_groups(two + [("@RG\\tID:a", "c.fa", None)], out=io.BytesIO()),           # an ID twice
                 lambda: al.align_groups([("@RG\\tID:a", None, None)], out=io.BytesIO()),
                 lambda: al.align_groups([("@RG\\tID:g%d\\tLB:l%d" % (k, k), "a.fa", None) for k in range(256)], out=io.BytesIO()),
                 lambda: al.align_groups(two, out=io.BytesIO(), fmt="bam", markdup=True),                 # markdup needs sort
                 lambda: al.align_groups(two, out=io.BytesIO(), fmt="bam", sort=True, markdup_metrics=io.StringIO()),
                 lambda: al.align_groups(two, out=io.StringIO(), fmt="bam")):
        with pytest.raises(ValueError):
            call()
    assert getattr(al, "_out_fmt", ("sam", 1)) == ("sam", 1) and not getattr(al, "_groups", None)
    al.rg_line = "@RG\tID:z"
    with pytest.raises(ValueError, match="-R is set"):
        al.align_groups(two, out=io.BytesIO())
    al.rg_line = ""
    al.profile = True
    with pytest.raises(NotImplementedError):
        al.align_groups(two, out=io.BytesIO())
    assert not getattr(al, "_groups", None)


def test_mem_command_refuses_misplaced_read_groups(capsys):
    from bwamem_hip import mem
    rg = "@RG\\tID:a"
    assert mem.main(["prefix", "early.fa", "--rg", rg, "a.fa"]) == 2
    assert "before the first --rg" in capsys.readouterr().err
    assert mem.main(["prefix", "--rg", rg, "--rg", "@RG\\tID:b", "b.fa"]) == 2
    assert "followed by 0 files" in capsys.readouterr().err
    assert mem.main(["prefix", "--rg", rg, "a_1.fq", "a_2.fq", "a_3.fq"]) == 2
    assert "followed by 3 files" in capsys.readouterr().err
    assert mem.main(["-R", "@RG\\tID:z", "prefix", "--rg", rg, "a.fa"]) == 2
    assert "--rg and -R exclude each other" in capsys.readouterr().err
    assert mem.main(["prefix", "--rg"]) == 2
    assert "--rg needs a value" in capsys.readouterr().err
