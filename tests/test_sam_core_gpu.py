"""The device side of the one SAM record writer (csrc/sam_core.h in csrc/sam_kernels.hip): the hand-made table of tests/sam_table.py through bmh_sam_select_device,
bmh_cigar_pack and the two text kernels against the lines written out there, and three cases aimed at the write kernel's paths (a wave's reads cut into parts, a
read beyond the wave's LDS share written to global memory directly, pieces that start at every byte of a dword) against the host formatter's text, which the CPU
tests pin.  288 reads in all."""
import numpy as np
import pytest

import sam_table
from sam_table import rec, read

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hip():
    import torch
    import bwamem_hip as B
    B.load_library()
    assert torch.cuda.is_available(), "these tests need a GPU"
    return B


def device_text(T, po, with_quals=False, with_comments=False) -> bytes:
    """records -> selection -> packed CIGARs -> text, all on the device; the selection and its slots must be the table's"""
    import torch
    from bwamem_hip.lib import cigar_pack, sam_select_device, sam_text_device
    t = lambda x, dt: torch.from_numpy(np.ascontiguousarray(x).astype(dt)).cuda()
    fin, fpr = t(T.fin.reshape(-1, 16), np.int32), t(T.fpr, np.int32)
    h = t(T.h_rec, np.int32) if T.paired else None
    sel, slot = sam_select_device(po, fin, fpr, h)
    assert np.array_equal(slot.cpu().numpy(), T.slot.astype(np.int32)) and np.array_equal(sel.cpu().numpy(), np.nonzero(T.need)[0])
    aln = t(T.aln.reshape(-1, 8), np.int32)
    off, packed = cigar_pack(aln, t(T.cigar.view(np.int32), np.int32), t(T.md, np.uint8))
    assert np.array_equal(off.cpu().numpy().view(np.uint32), T.cig_off) and np.array_equal(packed.cpu().numpy().view(np.uint32), T.packed[:-1])
    return sam_text_device(po, T.names, t(T.ascii, np.uint8), t(T.offs, np.int32), t(T.lens, np.int32), T.contigs, fin, fpr, slot, aln, off, packed,
                           h_rec_t=h, unflag_t=t(T.unflag, np.int32) if T.paired else None, quals_t=t(T.quals, np.uint8) if with_quals else None,
                           comments=T.comments if with_comments else None)


@pytest.mark.parametrize("case", list(sam_table.CASES))
def test_record_table_device_text_equals_lines(hip, case):
    reads, lines, opts, paired = sam_table.CASES[case]
    T = sam_table.Table(reads, flag_all=bool(opts.get("flag_all")), paired=paired)
    tags = "copy_comment" in opts
    got = device_text(T, sam_table.post_opt(opts), tags, tags)
    want = ("\n".join(lines) + "\n").encode()
    assert got == want, [(a, b) for a, b in zip(got.split(b"\n"), want.split(b"\n")) if a != b][:2]


def _bases(n, k):
    return "".join("ACGT"[(i * 7 + i // 5 + k) & 3] for i in range(n))


def _plain(name, k, L=150):
    """one forward record with soft clips, qualities and an XS"""
    return read(name, _bases(L, k), [rec(L - 10, ("c2", 11 + 3 * k, k & 1, "%dS%dM2I%dM" % (5, L - 47, 40), 2, "%dA%d" % (20, L - 28)), mapq=60 - k % 7, sub=k % 30)],
                qual="".join(chr(33 + (i + k) % 40) for i in range(L)))


def _same_as_host(T, po, **kw):
    got, want = device_text(T, po, **kw), T.host_text(po, **kw)
    assert got == want, (len(got), len(want), [(a, b) for a, b in zip(got.split(b"\n"), want.split(b"\n")) if a != b][:2])
    return want


def test_wave_beyond_its_lds_share_is_cut_into_parts(hip):
    """64 reads -- one wave -- whose records together exceed 16 384 bytes while each stays far below: names of about 200 bytes, 150-base reads with qualities"""
    reads = [_plain("n%02d_" % k + "x" * (190 + k % 9), k) for k in range(64)]
    want = _same_as_host(sam_table.Table(reads), sam_table.post_opt({}), with_quals=True)
    lens = [len(l) + 1 for l in want.split(b"\n")[:-1]]
    assert len(lens) == 64 and sum(lens) > 16384 + 3 and max(lens) < 1024


def test_one_read_beyond_the_lds_share_goes_to_global_memory(hip):
    """one read under flag_all with 48 reported records, every one with SEQ, QUAL and an SA tag that names the 47 others: its text exceeds 16 384 bytes"""
    L = 300
    recs = [rec(200 - j, ("c2" if j % 3 else "c1", 20 + 11 * j, j & 1, "%dS%dM%dS" % (j + 1, L - 2 * j - 2, j + 1), j % 5, "%d" % (L - 2 * j - 2)), mapq=j, flag=0x800 if j else 0,
                sub=j, sec=-1) for j in range(46)]
    recs += [rec(90, ("c2", 900, 0, "%dM" % L, 0, "%d" % L), mapq=0, flag=0x100, sec=0), rec(89, ("c2", 950, 1, "%dM" % L, 1, "%d" % L), mapq=0, flag=0x100, sec=0)]
    T = sam_table.Table([read("long_read_with_many_records", _bases(L, 1), recs, qual="".join(chr(40 + i % 30) for i in range(L)))], flag_all=True,
                        contigs=[("c1", 1000), ("c2", 2000)])
    want = _same_as_host(T, sam_table.post_opt(dict(flag_all=1)), with_quals=True)
    assert len(want) > 16384 and want.count(b"\n") == 48 and want.count(b"\tSA:Z:") == 46


def test_wave_pieces_start_at_every_byte_of_a_dword(hip):
    """193 reads in four waves: name lengths chosen so that the text of the first 64, 128 and 192 reads ends 1, 2 and 3 bytes behind a dword boundary -- the pieces
    of the second, third and fourth wave start there (the text buffer itself is aligned)"""
    probe = sam_table.Table([_plain("r", k, 50) for k in range(193)]).host_text(sam_table.post_opt({}), with_quals=True)
    lens = [len(l) + 1 for l in probe.split(b"\n")[:-1]]
    reads = [_plain("r" + "y" * (-lens[k] % 4 + (1 if k in (0, 64, 128) else 0)), k, 50) for k in range(193)]
    want = _same_as_host(sam_table.Table(reads), sam_table.post_opt({}), with_quals=True)
    ends = np.cumsum([len(l) + 1 for l in want.split(b"\n")[:-1]])
    assert [int(ends[k - 1]) & 3 for k in (64, 128, 192)] == [1, 2, 3]
