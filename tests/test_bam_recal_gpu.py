"""The recalibration table on the device: csrc/bam_recal_kernels.hip against the host form and against the Python model of tests/recal_model.py --
the table of cases (the hand-counted ones among them, their rows compared on the device too), synthetic records, every capacity of the kernel's form at its limit,
one below and one above (the slots, the lanes of a record, the cycles of an LDS row, the records of a block, the kept bases of a record that counts in LDS), read
groups that change inside a block and 255 of them, the refusals word for word, and the windows of the device merge
beside marking, coverage and the statistics with the BAM and its index byte for byte those of the run without the table."""
import numpy as np
import pytest

from recal_model import (ARRAYS, pack_pac, SMALL_CONTIGS, SMALL_LENS, SMALL_PAC, SMALL_REF, E_CUT, E_PLACEHOLDER, E_RG_ID, E_RG_NONE, E_RG_TYPE, E_SPAN, E_SUM, E_TAGS, I, M, S, WORDS, check_invariants, cut_record, equal, expect_rows, genome, hand_cases, mask_words, model, rrec,
                         synth_records, table_cases)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def G():
    contigs, ref, pac, hole = genome()
    mask = np.zeros(len(ref), bool); mask[hole[0]:hole[0] + hole[1]] = True; mask[::41] = True
    return dict(contigs=contigs, lens=[c[1] for c in contigs], ref=ref, pac=pac, mask=mask, words=mask_words(mask))


@pytest.fixture(scope="module")
def limits():
    from bwamem_hip.lib import recal_kernel_limits
    return recal_kernel_limits()


def three(G, recs, **kw):
    """device, host and model over one stream: the three are one table"""
    from bwamem_hip.lib import bam_recal
    s = b"".join(recs)
    dev = bam_recal(s, G["contigs"], G["pac"], len(G["ref"]), mask=G["words"], **kw)
    host = bam_recal(s, G["contigs"], G["pac"], len(G["ref"]), mask=G["words"], host=True, **kw)
    want = model(recs, G["lens"], G["ref"], G["mask"], groups=kw.get("read_groups"), min_qual=kw.get("min_qual", 6), max_cycle=kw.get("max_cycle", 500))
    for k in ARRAYS:
        assert np.array_equal(dev[k], host[k]), ("device != host", k, np.argwhere(dev[k] != host[k])[:4])
    assert equal(host, want)
    check_invariants(dev)
    return dev


def test_device_equals_host_equals_model_on_synthetic_records(G):
    recs = synth_records(3000, G["contigs"], G["ref"])
    r = three(G, recs)
    assert r["summary"][1] > 2500 and r["cycle_m"][..., 1].sum() > 0 and r["cycle_id"][..., 1].sum() > 0 and r["cycle_id"][..., 2].sum() > 0
    three(G, recs[:700], min_qual=0, max_cycle=37)
    three(G, [], max_cycle=1)


def small(mask=None):
    """the reference of the hand-counted cases as `three` takes it"""
    m = np.zeros(len(SMALL_REF), bool) if mask is None else mask
    return dict(contigs=SMALL_CONTIGS, lens=SMALL_LENS, ref=SMALL_REF, pac=SMALL_PAC, mask=m, words=mask_words(m))


def test_the_table_of_cases_on_the_device():
    """every case of the table -- clips, events at both ends in both strands, N, = and X, bases that are skipped for every reason, the caps, every reason a record
    is left out for -- device against host against model; the hand-counted ones give the rows written out by hand on the device too"""
    from bwamem_hip.recal import recal_table_text
    by_hand = {c[0]: c[4] for c in hand_cases()}
    for name, recs, mask, kw in table_cases():
        r = three(small(mask), recs, **kw)
        if name in by_hand:
            assert [ln for ln in recal_table_text(r).split("\n") if ln[:2] in ("CY", "CX")] == expect_rows(by_hand[name]), name
    # the same cases as one stream, so that the lanes of a block hold records of every kind side by side (one mask: the union would change the counts)
    for mask in (None, np.ones(len(SMALL_REF), bool)):
        three(small(mask), [r for _n, recs, _m, kw in table_cases() if not kw for r in recs] * 9)


def test_the_kept_bases_of_an_lds_record_at_the_limit(G, limits):
    """a record beyond the limit counts straight into the accumulator: its kept, skipped and capped words and every observation"""
    rng = np.random.default_rng(4)
    for n in (limits["lds_bases"] - 1, limits["lds_bases"], limits["lds_bases"] + 1):
        long_ref = np.concatenate([G["ref"], rng.integers(0, 4, n + 40, dtype=np.uint8)])
        seq = long_ref[len(G["ref"]) + 3:len(G["ref"]) + 3 + n].copy()
        seq[::97] = (seq[::97] + 1) % 4
        letters = np.array(list("ACGT"))[seq]; letters[5::1001] = "N"
        quals = [int(q) for q in rng.choice([3, 20, 30], n)]
        contigs = G["contigs"] + [("long", n + 40)]
        mask = np.zeros(len(long_ref), bool); mask[::211] = True
        g = dict(contigs=contigs, lens=[c[1] for c in contigs], ref=long_ref, pac=pack_pac(long_ref), mask=mask, words=mask_words(mask))
        recs = reads(G, 20, 30) + [rrec(b"long", 2, 3, fl, 30, ((2, S), (n - 1, M), (1, I), (1, S)), "AA" + "".join(letters) + "C", [30, 30] + quals + [30]) for fl in (0, 0x91)] + reads(G, 20, 30, flag=0x10)
        r = three(g, recs, max_cycle=300)
        assert int(r["summary"][12]) > 2 * (n - 400) * 0.5 and int(r["summary"][8]) > 0 and int(r["summary"][9]) > 0 and int(r["summary"][10]) > 0


def reads(G, n, length, quals=(30,), flag=0, start=0):
    """n records of `length` aligned bases cut from the first contig, the qualities cycling through `quals` base by base"""
    out = []
    for k in range(n):
        pos = (start + 7 * k) % (G["lens"][0] - length - 1)
        seq = "".join("ACGT"[c] for c in G["ref"][pos:pos + length])
        out.append(rrec(b"r%d" % k, 0, pos, flag, 30, ((length, M),), seq, [quals[(k + j) % len(quals)] for j in range(length)]))
    return out


def test_the_records_of_a_block_at_the_limit(G, limits):
    b = limits["block_records"]
    for n in (b - 1, b, b + 1, 2 * b + 3):
        r = three(G, reads(G, n, 20))
        assert int(r["summary"][0]) == n


def test_the_slots_at_the_limit(G, limits):
    """one group: every quality is a key and the indel row is one more"""
    for k in (limits["slots"] - 2, limits["slots"] - 1, limits["slots"], limits["slots"] + 9):
        r = three(G, reads(G, 40, 2 * k + 5, quals=tuple(range(6, 6 + k))))
        assert np.count_nonzero(r["cycle_m"][0, :, :, 0].sum(axis=1)) == k


def test_the_lanes_of_a_record_at_the_limit(G, limits):
    for n in (1, limits["lanes"] - 1, limits["lanes"], limits["lanes"] + 1, 2 * limits["lanes"] + 1):
        three(G, reads(G, 9, n) + reads(G, 9, n, flag=0x10) + [rrec(b"c", 0, 100, 0x91, 30, ((3, S), (n, M), (2, S)), "".join("ACGT"[c] for c in G["ref"][97:102 + n]), 30)])


def test_the_cycles_of_an_lds_row_at_the_limit(G, limits):
    for n in (limits["lds_cycles"] - 1, limits["lds_cycles"], limits["lds_cycles"] + 1, limits["lds_cycles"] + 40):
        r = three(G, reads(G, 5, n) + reads(G, 5, n, flag=0x81) + reads(G, 5, n, flag=0x91))
        assert int(r["summary"][12]) == 0
        r = three(G, reads(G, 5, n) + reads(G, 5, n, flag=0x81), max_cycle=limits["lds_cycles"])
        assert (int(r["summary"][12]) > 0) == (n > limits["lds_cycles"])


def test_groups_that_change_inside_a_block_and_255_groups(G):
    ids = ["g%d" % k for k in range(255)]
    recs = synth_records(900, G["contigs"], G["ref"], groups=ids, read_len=(20, 60))
    r = three(G, recs, read_groups=ids, max_cycle=64)
    assert np.count_nonzero(r["cycle_id"][:, :, 0].sum(axis=1)) > 200
    three(G, synth_records(600, G["contigs"], G["ref"], groups=ids[:3]), read_groups=ids[:3])


def test_the_refusals_word_for_word_and_the_smallest_index(G):
    from bwamem_hip.lib import bam_recal, bam_sorted_file
    ok = reads(G, 30, 25)
    bad_sum = rrec(b"x", 0, 5, 0, 30, ((10, M),), "ACGTACGTACG", 30)
    bad_span = rrec(b"y", 1, G["lens"][1] - 4, 0, 30, ((10, M),), "ACGTACGTAC", 30)
    stream = ok[:9] + [bad_span] + ok[9:20] + [bad_sum] + ok[20:]
    want = model(stream, G["lens"], G["ref"], G["mask"])
    assert want == ("refused", 9, E_SPAN)
    for host in (False, True):
        with pytest.raises(ValueError) as e:
            bam_recal(b"".join(stream), G["contigs"], G["pac"], len(G["ref"]), mask=G["words"], host=host)
        assert str(e.value) == "bmh_bam_recal: bmh_bam_recal_%s: record 9 %s" % ("host" if host else "device", WORDS[E_SPAN])
    grouped = [rrec(b"g%d" % k, 0, 5 + k, 0, 30, ((4, M),), "ACGT", 30, b"RGZa\0") for k in range(3)]
    for code, recs, groups in ((E_SUM, ok[:3] + [bad_sum], None), (E_RG_ID, grouped + [rrec(b"z", 0, 5, 0, 30, ((4, M),), "ACGT", 30, b"RGZnone\0")], ["a"]),
                               (E_RG_NONE, grouped + [ok[0]], ["a"]), (E_RG_TYPE, grouped + [rrec(b"z", 0, 5, 0, 30, ((4, M),), "ACGT", 30, b"RGi\1\0\0\0")], ["a"]),
                               (E_TAGS, ok[:3] + [rrec(b"z", 0, 5, 0, 30, ((4, M),), "ACGT", 30, b"XYZab")], None),
                               (E_PLACEHOLDER, ok[:3] + [rrec(b"z", 0, 5, 0, 30, ((4, S), (9, 3)), "ACGT", 30, b"CGBI\1\0\0\0\x40\0\0\0")], None),
                               (E_CUT, ok[:3] + [cut_record()], None)):
        msgs = []
        for host in (False, True):
            with pytest.raises(ValueError) as e:
                bam_recal(b"".join(recs), G["contigs"], G["pac"], len(G["ref"]), host=host, read_groups=groups)
            msgs.append(str(e.value).split(": ", 2)[2])
        assert msgs[0] == msgs[1] == "record 3 %s" % WORDS[code]
        assert model(recs, G["lens"], G["ref"], None, groups=groups) == ("refused", 3, code)
    # inside one window of the merge: two refused records, the one that comes first in the sorted file is named
    with pytest.raises(ValueError, match="record 3 begins or ends outside its contig"):
        bam_sorted_file("@CO\tx\n", G["contigs"], b"".join([bad_span, rrec(b"w", 1, G["lens"][1] - 2, 0, 30, ((10, M),), "ACGTACGTAC", 30)] + ok[:3]), 1, 0,
                        recal=dict(pac=G["pac"], l_pac=len(G["ref"])))


@pytest.mark.parametrize("window", (0, 1, 7, 25))
def test_the_windows_of_the_device_merge(G, window):
    from test_bam_sort import BamFile
    from bwamem_hip.lib import bam_sorted_file
    recs = synth_records(60, G["contigs"], G["ref"], seed=3, read_len=(20, 50))
    recs = [r[:18] + bytes([r[18] & 0x14, r[19] & 0x6]) + r[20:] for r in recs]         # (single reads: marking takes every name as one template)
    recs += [r[:36] + b"z" + r[37:] for r in recs[:6]]                         # (duplicates under other names for marking to find)
    s = b"".join(recs)
    kw = dict(pac=G["pac"], l_pac=len(G["ref"]), mask=G["words"])
    plain = bam_sorted_file("@CO\tx\n", G["contigs"], s, 1, window)
    bam, bai, got = bam_sorted_file("@CO\tx\n", G["contigs"], s, 1, window, recal=kw)
    assert (bam, bai) == plain
    assert equal(got, model(BamFile(bam).stream, G["lens"], G["ref"], G["mask"]))
    full = bam_sorted_file("@CO\tx\n", G["contigs"], s, 1, window, markdup=True, coverage={}, stats={})
    bam2, bai2, counts, cov, st, got2 = bam_sorted_file("@CO\tx\n", G["contigs"], s, 1, window, markdup=True, coverage={}, stats={}, recal=kw)
    assert (bam2, bai2, counts) == full[:3] and all(np.array_equal(cov[k], full[3][k]) for k in cov) and all(np.array_equal(st[k], full[4][k]) for k in st)
    assert equal(got2, model(BamFile(bam2).stream, G["lens"], G["ref"], G["mask"]))
    host = bam_sorted_file("@CO\tx\n", G["contigs"], s, 1, window, host=True, markdup=True, recal=kw)
    assert host[0] == bam2 and equal(host[-1], got2)
    flagged = sum(1 for r in BamFile(bam2).recs if r[19] & 0x4)
    assert flagged >= counts["records_flagged"] > 0                    # (the marked duplicates are counted out: the model reads the flags of the file)


def _reference(prefix, contigs):
    """the 2-bit codes of <prefix>.pac and the holes of <prefix>.amb as a boolean array"""
    from bwamem_hip.aligner import read_amb
    n = sum(c[1] for c in contigs)
    pac = np.fromfile(prefix + ".pac", dtype=np.uint8)[:(n + 3) // 4]
    codes = np.stack([pac >> 6 & 3, pac >> 4 & 3, pac >> 2 & 3, pac & 3], axis=1).reshape(-1)[:n]
    holes = np.zeros(n, bool)
    for a, b in read_amb(prefix):
        holes[a:a + b] = True
    return codes, holes


def _a_mismatch(recs, lens, ref):
    """the genome position of a mismatch under M of a counted, gap-free forward record"""
    import struct
    starts = np.concatenate([[0], np.cumsum(lens)])
    for r in recs:
        rid, pos, l_name, mapq, _bin, n_ops, fl, l_seq = struct.unpack_from("<iiBBHHHI", r, 4)
        if rid < 0 or fl & 0xf14 or not 0 < mapq < 255 or n_ops != 1 or struct.unpack_from("<I", r, 36 + l_name)[0] != l_seq << 4:
            continue
        at = 36 + l_name + 4
        for i in range(l_seq):
            c = {1: 0, 2: 1, 4: 2, 8: 3}.get(r[at + i // 2] >> (0 if i & 1 else 4) & 15, -1)
            if c >= 0 and c != ref[starts[rid] + pos + i] and r[at + (l_seq + 1) // 2 + i] >= 6:
                return rid, pos + i
    raise AssertionError("no mismatch among the records")


def test_reads_to_sorted_bam_with_its_recalibration_table(tmp_path):
    import io
    from test_bam_dup_gpu import _dup_reads
    from test_bam_gpu import PREFIX
    from test_bam_sort import BamFile
    from bwamem_hip.aligner import Aligner
    from bwamem_hip.bam import bam_post_file
    from bwamem_hip.recal import read_recal_table, recal_table_text
    reads = _dup_reads(tmp_path, True)[0]
    al = Aligner(PREFIX, n_threads=4)
    try:
        def run(**kw):
            out, idx = io.BytesIO(), io.BytesIO()
            al.align_files(reads, out=out, fmt="bam", sort=True, index=idx, paired=True, markdup=True, batch_reads=256, sort_window=7, **kw)
            return out.getvalue(), idx.getvalue()
        plain = run()
        text = io.StringIO()
        assert run(recal=text) == plain                                       # the BAM and its index are those of the run without the table
        lens = [c[1] for c in al.contigs]
        ref, holes = _reference(PREFIX, al.contigs)
        recs = BamFile(plain[0]).recs
        want = model(recs, lens, ref, holes)
        assert equal(al.recal, want) and text.getvalue() == recal_table_text(dict(want, min_qual=6, max_cycle=500, read_groups=["*"], known_sites=[]))
        check_invariants(al.recal)
        assert al.markdup_counts["records_flagged"] > 0 and int(want["summary"][3]) >= al.markdup_counts["records_flagged"] and int(want["summary"][1]) > 100
        assert int(want["cycle_m"][..., 1].sum()) > 0 and (want["cycle_m"][0, :, :500, 0].sum() > 0) and (want["cycle_m"][0, :, 500:, 0].sum() > 0)
        # a known site at a mismatch: exactly what the model loses there is lost
        rid, p = _a_mismatch(recs, lens, ref)
        bed = tmp_path / "known.bed"
        bed.write_text("%s\t%d\t%d\n" % (al.contigs[rid][0], p, p + 1))
        masked = holes.copy(); masked[sum(lens[:rid]) + p] = True
        text2 = io.StringIO()
        assert run(recal=text2, known_sites=[str(bed)]) == plain
        want2 = model(recs, lens, ref, masked)
        assert equal(al.recal, want2) and int(want2["cycle_m"][..., 1].sum()) < int(want["cycle_m"][..., 1].sum()) and int(want2["summary"][10]) > int(want["summary"][10])
        assert equal(read_recal_table(text2.getvalue().split("\n")), want2) and "AR\tknown_sites\t%s" % bed in text2.getvalue()
        assert run() == plain                                                 # switched off again
        with pytest.raises(ValueError, match="need sort=True"):
            al.align_files(reads, out=io.BytesIO(), fmt="bam", paired=True, recal=io.StringIO())
        # the same text from the unsorted BAM of that run, against the reference's files
        ubam = str(tmp_path / "u.bam")
        with open(ubam, "wb") as f:
            al.align_files(reads, out=f, fmt="bam", paired=True, batch_reads=256)
        for host in (False, True):
            got, o, i = io.StringIO(), io.BytesIO(), io.BytesIO()
            r = bam_post_file(ubam, o, index=i, host=host, markdup=True, sort_window=7, recal=got, reference=PREFIX, known_sites=[str(bed)])
            assert (o.getvalue(), i.getvalue()) == plain and got.getvalue() == text2.getvalue() and equal(r["recal"], want2), host
    finally:
        al.close()


def test_a_run_that_keeps_its_inputs_read_groups(tmp_path):
    """keep_rg=True: the table's groups are the @RG lines of the input's header, read ahead of the run; every record's RG:Z finds its group"""
    import io
    from test_bam_sort import BamFile
    from test_keep_rg_gpu import IDS3, LINES3, PREFIX, _fastx, _input_bam, _reads_files
    from bwamem_hip.aligner import Aligner
    reads_ = _fastx(_reads_files(tmp_path, True, n=300))
    bam = _input_bam(tmp_path, "in.bam", reads_, True, lambda t: IDS3[t % 3], LINES3)
    al = Aligner(PREFIX, n_threads=4)
    try:
        def run(**kw):
            out = io.BytesIO()
            al.align_files(bam, out=out, fmt="bam", sort=True, keep_rg=True, batch_reads=64, **kw)
            return out.getvalue()
        plain, text = run(), io.StringIO()
        assert run(recal=text) == plain
        ref, holes = _reference(PREFIX, al.contigs)
        want = model(BamFile(plain).recs, [c[1] for c in al.contigs], ref, holes, groups=list(IDS3))
        assert equal(al.recal, want) and al.recal["read_groups"] == list(IDS3)
        assert all(int(v) > 0 for v in al.recal["cycle_id"][:, :, 0].sum(axis=1)) and [ln for ln in text.getvalue().split("\n") if ln.startswith("AR\tread_group")] == ["AR\tread_group\t" + g for g in IDS3]
        with pytest.raises(ValueError, match="a BAM file, not a pipe"):
            al.align_files("/dev/stdin", out=io.BytesIO(), fmt="bam", sort=True, keep_rg=True, recal=io.StringIO())
    finally:
        al.close()


def test_an_aligner_in_memory_with_a_planted_variant(tmp_path):
    """Aligner.from_memory (no index files: no holes), pairs drawn from a genome that differs from the reference at one position, every fifth pair twice: the table
    is the model's over the file written; masking the variant's position removes exactly its errors; the marked duplicates are counted out"""
    import io
    import struct
    import common
    from test_bam_sort import BamFile
    from bwamem_hip import synth
    from bwamem_hip.aligner import Aligner
    g, idx = common.genome_and_index(20_000)
    V, n_pairs, L = 10_007, 1200, 100
    alt = np.array(g).copy(); alt[V] = (alt[V] + 1) % 4
    pairs = synth.make_pairs(alt, n_pairs, L, seed=11, sub_rate=0.005)[0]
    asc = [synth.codes_to_ascii(np.asarray(r)).tobytes() for r in pairs]
    quals = [bytes(q) for q in synth.random_quals([len(a) for a in asc], seed=11)]
    fq = tmp_path / "planted.fq"
    with open(fq, "wb") as f:
        for copy in range(2):
            for t in range(n_pairs):
                if copy and t % 5:
                    continue
                for m in (0, 1):
                    f.write(b"@p%d_%d/%d\n" % (t, copy, m + 1) + asc[2 * t + m] + b"\n+\n" + quals[2 * t + m] + b"\n")
    al = Aligner.from_memory(idx, g, n_threads=4)
    try:
        def run(**kw):
            out = io.BytesIO()
            al.align_files(str(fq), out=out, paired=True, fmt="bam", sort=True, markdup=True, **kw)
            return out.getvalue()
        plain, text = run(), io.StringIO()
        assert run(recal=text) == plain
        recs = BamFile(plain).recs
        lens, ref = [c[1] for c in al.contigs], np.asarray(g, dtype=np.uint8)
        want = model(recs, lens, ref, None)
        assert equal(al.recal, want) and int(want["summary"][13]) == 0
        flagged = sum(1 for r in recs if struct.unpack_from("<H", r, 18)[0] & 0x400)
        left_out = sum(1 for r in recs if struct.unpack_from("<i", r, 4)[0] >= 0 and struct.unpack_from("<H", r, 18)[0] & 0x704)
        assert flagged == al.markdup_counts["records_flagged"] > 100 and int(want["summary"][3]) == left_out >= flagged
        bed = tmp_path / "variant.bed"
        bed.write_text("%s\t%d\t%d\n" % (al.contigs[0][0], V, V + 1))
        assert run(recal=io.StringIO(), known_sites=[str(bed)]) == plain
        mask = np.zeros(len(ref), bool); mask[V] = True
        want2 = model(recs, lens, ref, mask)
        lost = int(want["cycle_m"][..., 1].sum()) - int(want2["cycle_m"][..., 1].sum())
        assert equal(al.recal, want2) and int(al.recal["summary"][13]) == 1
        # nothing else went with the mask: the observations lost are the bases skipped for it, and all of them but a sequencing error or two were errors
        gone = int(want["cycle_m"][..., 0].sum()) - int(want2["cycle_m"][..., 0].sum())
        assert gone == int(want2["summary"][10]) and 5 < gone - 2 <= lost <= gone
    finally:
        al.close()
