"""Applying a recalibration table to the base qualities on the device: csrc/bam_requal_kernels.hip against the host form and against the Python
model of tests/requal_model.py -- the qualities listed by hand, synthetic records, the lanes of a record and the records of a block at their limits, quality
fields at every alignment with their neighbours' bytes, a record beyond the LDS counts, 255 read groups, the refusals, the windows of the device merge beside
marking, coverage, the statistics and the counting of a table, and an aligner's runs."""
import io
import struct

import numpy as np
import pytest

from recal_model import E_CUT, E_RG_ID, E_RG_NONE, E_RG_TYPE, E_TAGS, equal, genome, synth_records
from requal_model import WORDS, apply_model, random_table, same_counts, split
from test_bam_requal import HAND, delta_table, hand_table, only_qualities_differ, quals, read

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def limits():
    from bwamem_hip.lib import requal_kernel_limits
    return requal_kernel_limits()


@pytest.fixture(scope="module")
def T():
    return random_table(3)


def three(recs, table):
    """device, host and model over one stream: the three give one stream and one set of counts"""
    from bwamem_hip.lib import bam_apply_recal, recal_apply_tables
    s = b"".join(recs)
    dev, dc = bam_apply_recal(s, table)
    host, hc = bam_apply_recal(s, table, host=True)
    want, wc = apply_model(recs, table, recal_apply_tables(table))
    assert dev == host, "device != host"
    assert host == b"".join(want) and same_counts(hc, wc)
    assert same_counts(dc, wc), (dc["summary"][:9], wc["summary"][:9])
    return split(dev), dc


def test_device_equals_host_equals_model(T):
    contigs, ref, _pac, _hole = genome()
    got, c = three(synth_records(3000, contigs, ref), T)
    assert c["bases_changed"] > 50_000 and c["records_without_qualities"] > 0 and c["bases_below_min_qual"] > 0
    ids = ["lane1", "lane2", "x"]
    three(synth_records(700, contigs, ref, seed=2, groups=ids), random_table(4, ids, max_cycle=37))
    three([], T)
    # the qualities listed by hand, on the device
    got, _c = three([rec for _w, rec, _q in HAND[:-1]], hand_table())
    assert [quals(r) for r in got] == [q for _w, _r, q in HAND[:-1]]
    got, _c = three([read("ACGT", [30, 25, 93, 6]), read("AC", [94, 255]), read("ACG", [5, 0, 7]), read("ACG", None), read("", None)], delta_table())
    assert [quals(r) for r in got] == [[20, 15, 83, 1], [83, 83], [5, 0, 1], [0xff] * 3, []]


def _reads(n, length, seed, flags=(0, 0x10, 0x81, 0x91), name_len=None):
    rng = np.random.default_rng(seed)
    out = []
    for k in range(n):
        seq = "".join("ACGTN"[c] for c in rng.choice(5, length, p=[.245, .245, .245, .245, .02]))
        name = (b"%d" % k).rjust(name_len, b"n")[:name_len] if name_len else b"q%d" % k
        out.append(read(seq, [int(q) for q in rng.choice([2, 6, 7, 11, 25, 37, 40, 41, 60], length)], flags[k % len(flags)], name=name))
    return out


def test_the_lanes_of_a_record_and_the_records_of_a_block_at_their_limits(T, limits):
    lanes, block = limits["lanes"], limits["block_records"]
    assert lanes == 16 and block % (256 // lanes) == 0
    for n in (1, lanes - 1, lanes, lanes + 1, 2 * lanes + 1):
        three(_reads(8, n, n), T)
    for n in (block - 1, block, block + 1):
        got, c = three(_reads(n, 21, n), T)
        assert c["records_seen"] == n


def test_quality_fields_at_every_alignment_leave_their_neighbours_alone(T):
    """read names of 1 .. 8 bytes and odd lengths: the quality field starts at every alignment modulo 8, and the records lie back to back"""
    recs = [r for name_len in range(1, 9) for r in _reads(9, 13 + name_len, name_len, name_len=name_len)]
    starts = np.cumsum([0] + [len(r) for r in recs])[:-1]
    at = {int(s + 36 + r[12] + 4 + (struct.unpack_from("<I", r, 20)[0] + 1) // 2) % 8 for s, r in zip(starts, recs)}
    assert at == set(range(8))
    got, _c = three(recs, T)
    assert all(only_qualities_differ(a, b) for a, b in zip(recs, got)) and any(a != b for a, b in zip(recs, got))


def test_a_record_beyond_the_lds_counts(T, limits):
    n = limits["lds_bases"]
    assert n == 65536
    got, c = three(_reads(1, n + 1, 1) + _reads(1, n, 2, flags=(0x91,)) + _reads(3, 40, 3), T)
    # (capped: the bases beyond cycle 500 at or above min_qual -- 8 of the 9 qualities drawn: about 8 / 9 of 2 (n - 500); three() has compared the count itself with the model)
    assert c["bases_seen"] == 2 * n + 1 + 120 and c["cycles_capped"] > 2 * (n - 500) * 0.8


def test_255_groups_that_change_record_by_record():
    ids = ["g%d" % k for k in range(255)]
    t = random_table(5, ids, max_cycle=8, cycles=8, quals=(25, 40))
    rng = np.random.default_rng(5)
    recs = [read("".join("ACGT"[c] for c in rng.integers(0, 4, 12)), [int(q) for q in rng.choice([25, 40], 12)], (0, 0x91)[k & 1], tag=b"RGZ" + ids[(7 * k) % 255].encode() + b"\0")
            for k in range(600)]
    three(recs, t)


def test_the_refusals_and_the_smallest_index_of_a_window(limits):
    from bwamem_hip.lib import bam_apply_recal
    ids = ["lane1", "lane2"]
    t = random_table(8, ids, max_cycle=20, cycles=20)
    ok = read("ACGT", 30, tag=b"RGZlane2\0")
    bad = {E_TAGS: read("ACGT", 30, tag=b"RGZlane1"), E_RG_NONE: read("ACGT", 30, tag=b"NMC\x01"), E_RG_TYPE: read("ACGT", 30, tag=b"RGA1"), E_RG_ID: read("ACGT", 30, tag=b"RGZlane3\0"),
           E_CUT: (lambda r: r[:20] + struct.pack("<I", 40) + r[24:])(read("ACGT", 30, tag=b"RGZlane1\0"))}
    for code, rec in bad.items():
        for host in (False, True):
            with pytest.raises(ValueError) as e:
                bam_apply_recal(ok + ok + rec + ok, t, host=host)
            assert str(e.value) == "bmh_bam_requal: bmh_bam_requal_%s: record 2 " % ("host" if host else "device") + WORDS[code], code
    # refused records in two blocks of one window: the smallest index, whichever block comes first
    n = limits["block_records"]
    with pytest.raises(ValueError, match="record 3 has no RG tag"):
        bam_apply_recal(b"".join([ok] * 3 + [bad[E_RG_NONE]] + [ok] * n + [bad[E_RG_ID]] + [ok] * 5 + [bad[E_TAGS]]), t)


@pytest.mark.parametrize("window", (0, 1, 7, 25))
def test_the_windows_of_the_device_merge(T, window):
    from test_bam_sort import BamFile
    from bwamem_hip.lib import bam_recal, bam_sorted_file
    contigs, ref, pac, _hole = genome()
    recs = synth_records(60, contigs, ref, seed=3, read_len=(20, 50))
    recs = [r[:18] + bytes([r[18] & 0x14, r[19] & 0x6]) + r[20:] for r in recs]          # (single reads: marking takes every name as one template)
    recs += [r[:36] + b"z" + r[37:] for r in recs[:6]]                                  # (duplicates under other names for marking to find)
    s = b"".join(recs)
    plain = bam_sorted_file("@CO\tx\n", contigs, s, 1, window)
    bam, _ix, got = bam_sorted_file("@CO\tx\n", contigs, s, 1, window, apply_recal=T)
    want, wc = apply_model(BamFile(plain[0]).stream, T)
    assert BamFile(bam).stream == b"".join(want) and same_counts(got["apply"], wc)
    assert (bam, _ix) == bam_sorted_file("@CO\tx\n", contigs, s, 1, window, host=True, apply_recal=T)[:2]
    # beside marking, coverage, the statistics and the counting of a table, which all see the qualities as written
    kw = dict(pac=pac, l_pac=len(ref))
    full = bam_sorted_file("@CO\tx\n", contigs, s, 1, window, markdup=True, coverage={}, stats={})
    bam2, ix2, counts, cov, st, rc = bam_sorted_file("@CO\tx\n", contigs, s, 1, window, markdup=True, coverage={}, stats={}, recal=kw, apply_recal=T)
    want2, wc2 = apply_model(BamFile(full[0]).stream, T)
    assert BamFile(bam2).stream == b"".join(want2) and same_counts(rc["apply"], wc2) and counts == full[2] and counts["records_flagged"] > 0
    assert all(np.array_equal(cov[k], full[3][k]) for k in cov)                          # (coverage reads no quality)
    assert equal(rc, bam_recal(BamFile(bam2).stream, contigs, pac, len(ref), host=True))
    host = bam_sorted_file("@CO\tx\n", contigs, s, 1, window, host=True, markdup=True, coverage={}, stats={}, recal=kw, apply_recal=T)
    assert host[:3] == (bam2, ix2, counts) and equal(host[-1], rc) and same_counts(host[-1]["apply"], wc2) and all(np.array_equal(st[k], host[4][k]) for k in st)


def test_an_aligner_counts_a_table_then_applies_it(tmp_path):
    """Aligner.from_memory: a first run counts the table of its sorted, marked file; a second applies it -- the records but for their qualities, the 0x400 flags and
    the duplicate counts are the first run's, the qualities the model's; bam_post_file gives the second run's file from the first's unsorted BAM; a third run
    counts the "after" table beside the applying"""
    import common
    from test_bam_sort import BamFile
    from bwamem_hip import synth
    from bwamem_hip.aligner import Aligner
    from bwamem_hip.bam import bam_post_file
    from bwamem_hip.lib import bam_recal
    from bwamem_hip.recal import read_recal_table
    g, idx = common.genome_and_index(20_000)
    n_pairs, L = 400, 100
    pairs = synth.make_pairs(np.array(g), n_pairs, L, seed=11, sub_rate=0.01)[0]
    asc = [synth.codes_to_ascii(np.asarray(r)).tobytes() for r in pairs]
    qs = [bytes(q) for q in synth.random_quals([len(a) for a in asc], seed=11)]
    fq = tmp_path / "reads.fq"
    with open(fq, "wb") as f:
        for copy in range(2):
            for t in range(n_pairs):
                if copy and t % 5:
                    continue
                for m in (0, 1):
                    f.write(b"@p%d_%d/%d\n" % (t, copy, m + 1) + asc[2 * t + m] + b"\n+\n" + qs[2 * t + m] + b"\n")
    al = Aligner.from_memory(idx, g, n_threads=4)
    try:
        def run(**kw):
            out, ix = io.BytesIO(), io.BytesIO()
            al.align_files(str(fq), out=out, paired=True, fmt="bam", sort=True, index=ix, markdup=True, sort_window=300, **kw)
            return out.getvalue(), ix.getvalue()
        text = io.StringIO()
        first = run(recal=text)
        counts1 = dict(al.markdup_counts)
        t = read_recal_table(text.getvalue().split("\n"))
        report = io.StringIO()
        second = run(apply_recal=t, apply_recal_report=report)
        a, b = BamFile(first[0]).recs, BamFile(second[0]).recs
        want, wc = apply_model(a, t)
        assert b == want and same_counts(al.recal_apply, wc) and wc["summary"][5] > 10_000
        assert all(only_qualities_differ(x, y) for x, y in zip(a, b)) and al.markdup_counts == counts1 and counts1["records_flagged"] > 50
        assert report.getvalue().startswith("AS\trecords_seen\t%d\n" % len(a))
        assert run() == first                                                        # switched off again: the file of the run without the option
        ubam = str(tmp_path / "u.bam")
        with open(ubam, "wb") as f:
            al.align_files(str(fq), out=f, paired=True, fmt="bam")
        for host in (False, True):
            o, i = io.BytesIO(), io.BytesIO()
            r = bam_post_file(ubam, o, index=i, host=host, markdup=True, sort_window=300, apply_recal=t)
            assert (o.getvalue(), i.getvalue()) == second and same_counts(r["recal_apply"], wc), host
        # the "after" table beside the applying
        text2 = io.StringIO()
        third = run(apply_recal=t, recal=text2)
        lens = [c[1] for c in al.contigs]
        assert third == second and same_counts(al.recal_apply, wc)
        assert equal(al.recal, bam_recal(b"".join(b), lens, al.pac, al.l_pac, host=True)) and equal(read_recal_table(text2.getvalue().split("\n")), al.recal)
        assert not np.array_equal(al.recal["cycle_m"], t["cycle_m"])
        with pytest.raises(ValueError, match="apply_recal needs sort=True"):
            al.align_files(str(fq), out=io.BytesIO(), fmt="bam", paired=True, apply_recal=t)
    finally:
        al.close()
