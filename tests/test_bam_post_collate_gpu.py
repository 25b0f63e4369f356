"""Mark duplicates in a file that is not grouped by name, on the device (BDP_TPL_FILE): bam_templates on the device equals the host form integer
for integer on test_bam_post_collate.py's case table and at the structural edges of csrc/bam_tpl_kernels.hip (a block's edge, a set longer than a block, mates at
both ends of the file, every option, forced collisions), the edges also against the model; bam_post_file(collate=True) on the device equals the host form byte for
byte on the permuted golden and synthetic files at every batch_bytes, with libraries, optical and barcode counts and coverage; the refusals' words equal the host
form's; and end to end: this aligner's own --sort output through the tool with --markdup --collate gives the counts of its own --sort --markdup run."""
import io

import numpy as np
import pytest

import common
from test_bam_dup import pair, rec, synthetic
from test_bam_post import CONTIGS, HEADER, bam_file, post, sup
from test_bam_post_collate import (FOUR, GROUPS, collate_model, first_record_cases, model_entries, orders, permuted_corpus, refusal_cases, table, tagged)
from test_bam_post_gpu import _reads, same
from test_bam_sort import check_file, py_sort, split_records


@pytest.fixture(scope="module")
def hip():
    import torch
    import bwamem_hip as B
    B.load_library()
    assert torch.cuda.is_available(), "these tests need a GPU"
    return B


def same_templates(stream, what, model=False, **kw):
    from bwamem_hip.lib import bam_templates
    d, h = bam_templates(stream, host=False, **kw), bam_templates(stream, host=True, **kw)
    assert sorted(d) == sorted(h), what
    for k in h:
        if isinstance(h[k], np.ndarray):
            assert d[k].dtype == h[k].dtype and np.array_equal(d[k], h[k]), (what, k)
        else:
            assert d[k] == h[k], (what, k)
    if model:
        tpl, entries = model_entries(split_records(stream))
        assert d["tpl"].tolist() == tpl and [tuple(int(v) for v in x) for x in d["entries"]] == entries, what
    return d


def singles(n):
    return [rec(b"one%d" % i, 1, 100 + 7 * (i % 40), 16 * (i % 2), q=10 + i % 30) for i in range(n)]


def edges():
    """(what, stream): the record counts around a block's edge, a set longer than a wave and a block, mates at index 0 and N - 1"""
    E = [("%d single-record templates" % n, b"".join(singles(n))) for n in (1, 255, 256, 257)]
    E.append(("one name holding 257 records", b"".join([sup(b"long", 0, 10 + i) for i in range(200)] + [rec(b"long", 1, 500, 0)] + [sup(b"long", 0, 900 + i) for i in range(56)])))
    m = pair(b"ends", 1, 100, False, 1, 300, True)
    E.append(("mates at index 0 and N - 1", b"".join([m[0]] + singles(255) + [m[1]])))
    E.append(("synthetic 300, coordinate-sorted", py_sort(synthetic(300, 11))))
    return E


@pytest.mark.gpu
@pytest.mark.parametrize("case", table(), ids=lambda c: c[0])
def test_templates_device_equals_host_on_the_case_table(hip, case):
    same_templates(b"".join(case[1]), case[0], model=True)


@pytest.mark.gpu
@pytest.mark.parametrize("case", edges(), ids=lambda c: c[0])
def test_templates_at_the_structural_edges(hip, case):
    what, stream = case
    d = same_templates(stream, what, model=True)
    if what.startswith("one name"):
        assert d["counts"] == dict(secondary_or_supplementary=256, unmapped_records=0, templates=1) and int(d["entries"][0]["kind_n"]) == 1 | 257 << 2


def illumina(n_pairs=150, seed=5):
    """pairs under seven-field names on few positions and tiles, with RG:Z and RX:Z on both records: duplicates, optical duplicates, libraries and barcodes"""
    rng = np.random.default_rng(seed)
    out = []
    for t in range(n_pairs):
        p = 1000 + 500 * int(rng.integers(0, 12))
        name = b"M1:7:FC:1:%d:%d:%d" % (1101 + t % 2, 1000 + 3 * t, 2000 + 40 * int(rng.integers(0, 8)))       # (x makes the names distinct)
        tags = b"RGZ" + (b"a", b"b", b"c")[t % 3] + b"\0" + (b"RXZ" + (b"ACGTAC", b"ACGTAA", b"TTGACA")[int(rng.integers(0, 3))] + b"\0" if t % 4 else b"")
        out += [tagged(r, tags) for r in pair(name, 1, p, False, 1, p + 200, True, q=int(rng.integers(10, 40)))]
    return b"".join(out)


RG_HEADER = HEADER + "".join(f"@RG\tID:{i}\tLB:{l}\n" for i, l in GROUPS)


@pytest.mark.gpu
def test_templates_with_every_option(hip):
    stream = py_sort(illumina())
    for kw in (dict(read_groups=GROUPS), dict(barcode_tag="RX"), dict(barcode_name=True), dict(barcode_tag="RX", barcode_edits=1), dict(read_groups=GROUPS, barcode_tag="RX")):
        d = same_templates(stream, kw, **kw)
        assert d["counts"]["templates"] == 150 and ("barcode_name" in kw or int((d["locations"]["flags"] & 1).sum()) == 150)
    d = same_templates(first_record_cases()[0], "first records", read_groups=GROUPS, barcode_tag="RX")
    assert [int(e["lo"]) >> 56 for e in d["entries"]] == first_record_cases()[1] and [int(w) for w in d["barcodes"]] == first_record_cases()[2]


@pytest.mark.gpu
def test_forced_collisions(hip):
    from bwamem_hip.lib import bam_templates
    stream = b"".join(r for i in range(300) for r in pair(b"n%d" % i, 1, 100 + i, False, 1, 400 + i, True))
    same_templates(stream, "64 bits", hash_bits=64)
    same_templates(stream, "127 bits", hash_bits=127)
    for bits in (1, 5):
        words = []
        for host in (True, False):
            with pytest.raises(ValueError, match=r"hold \d+ primary lines") as e:
                bam_templates(stream, host=host, hash_bits=bits)
            words.append(str(e.value).replace("_device", "_host"))
        assert words[0] == words[1], bits


@pytest.mark.gpu
@pytest.mark.parametrize("k", range(3))
def test_post_device_equals_host_on_permuted_files(hip, tmp_path, k):
    what, contigs, header, stream = permuted_corpus()[k]
    for order, s in orders(stream, 5 + k).items():
        path = bam_file(tmp_path / "in.bam", header, contigs, s)
        for bb in (1, 200, None):
            host = post(path, host=True, markdup=True, collate=True, coverage=io.StringIO(), batch_bytes=bb)
            same(post(path, host=False, markdup=True, collate=True, coverage=io.StringIO(), batch_bytes=bb), host, (what, order, bb))
    hdr, recs, c, m = collate_model(header, s)
    check_file(host[0], host[1], hdr, contigs, b"".join(recs), what, n_regions=0)


@pytest.mark.gpu
def test_post_device_equals_host_with_libraries_optical_barcodes_and_spilling(hip, tmp_path):
    s = py_sort(illumina())
    path = bam_file(tmp_path / "in.bam", RG_HEADER, CONTIGS, s)
    kw = dict(markdup=True, collate=True, libraries=True, optical_distance=100, barcode_tag="RX", coverage=io.StringIO())
    host = post(path, host=True, **kw)
    md = host[2]["markdup"]
    assert md["duplicate_pairs"] > 0 and md["optical_duplicate_pairs"] > 0 and md["templates_without_barcode"] > 0 and len(md["libraries"]) == 2
    for bb in (1, 200, None):
        same(post(path, host=False, batch_bytes=bb, **kw), post(path, host=True, batch_bytes=bb, **kw), bb)
    kw.update(barcode_edits=1, index_format="csi")
    same(post(path, host=False, **kw), post(path, host=True, **kw), "edits, csi")
    spilled = post(path, host=False, batch_bytes=4096, sort_mem=1, **kw)
    held = post(path, host=True, batch_bytes=4096, **kw)
    assert spilled[2]["counts"].pop("spilled_runs") == spilled[2]["counts"]["batches"] > 1 and held[2]["counts"].pop("spilled_runs") == 0
    same(spilled, held, "spilled")
    # the name-grouped file: the option changes nothing on the device either
    grouped = bam_file(tmp_path / "g.bam", RG_HEADER, CONTIGS, illumina())
    kw.pop("collate")
    same(post(grouped, host=False, collate=True, **kw), post(grouped, host=False, **kw), "name-grouped")


@pytest.mark.gpu
@pytest.mark.parametrize("which", sorted(refusal_cases()))
def test_refusal_messages_equal_the_host_forms(hip, tmp_path, which):
    from bwamem_hip.bam import bam_post_file
    stream, _match, kw = refusal_cases()[which]
    kw = dict(kw)
    path = bam_file(tmp_path / "bad.bam", kw.pop("header", HEADER), CONTIGS, stream)
    for bb in (None, 1):
        words = []
        for host in (True, False):
            out = io.BytesIO()
            with pytest.raises(ValueError) as e:
                bam_post_file(path, out, host=host, markdup=True, collate=True, batch_bytes=bb, **kw)
            assert out.getvalue() == b""
            words.append(str(e.value).replace("_device", "_host"))
        assert words[0] == words[1], (which, bb)
    with pytest.raises(ValueError, match="collate needs marking"):
        bam_post_file(path, io.BytesIO(), host=False, collate=True)


@pytest.mark.gpu
def test_the_aligners_sorted_output_through_the_tool(hip, tmp_path):
    from bwamem_hip.aligner import Aligner
    g, idx = common.genome_and_index(20_000)
    fq = _reads(tmp_path, g)
    al = Aligner.from_memory(idx, g, n_threads=4)
    try:
        plain, marked = io.BytesIO(), io.BytesIO()
        al.align_files(fq, out=plain, paired=True, fmt="bam", sort=True, index=io.BytesIO())
        al.align_files(fq, out=marked, paired=True, fmt="bam", sort=True, index=io.BytesIO(), markdup=True)
        counts = dict(al.markdup_counts)
        assert counts["duplicate_pairs"] > 20
        path = tmp_path / "sorted.bam"
        path.write_bytes(plain.getvalue())
        r = post(str(path), host=False, markdup=True, collate=True)[2]
        assert {c: r["markdup"][c] for c in FOUR} == {c: counts[c] for c in FOUR}
    finally:
        al.close()
