"""Single-end `gase_aln` on the device-resident path: index files + FASTA or FASTQ reads -> SAM.

The reference's CLI keeps working on this library through the drop-in headers (INTEGRATION.md sections 1-2); this module
is the same job done through the device-level C ABI instead -- seeding, chaining / job construction, extension and the
region merge on the GPU (bmh_seed_batch, bmh_chain_batch, bmh_chain_extend, bmh_chain_merge), the region tail on host
threads as in the reference (bmh_finalize_regs), CIGAR / NM / MD on the GPU (bmh_cigar_batch), SAM text on the host
(bmh_format_sam).  It writes the records the reference writes, byte for byte (tests/test_gpu_parity.py).  torch is used
for device memory only.  Interleaved pairs (gase_aln -p) go through bmh_finalize_pairs / bmh_format_sam_pe; their
insert-size statistics are per batch as in the reference, so identical output needs the reference's batching (one batch
here = batch_reads reads).  ALT contigs come from <prefix>.alt as in the reference; read groups come from -R.  FASTQ files (four-line
records) give QUAL as the reference writes it (src/bwamem.c:1575-1612), and -C appends every read's header comment (src/bwamem.c:1670-1673);
a FASTA file still gives QUAL '*'.
"""
from __future__ import annotations

import ctypes as C
import functools
import inspect
import os

import numpy as np
import torch

from . import fmindex
from .lib import (EXT_LONG_MAX, ChainOpt, ChainWorkspace, ExtParams, Index, PeOpt, PostOpt, ReseedOpt, SeedWorkspace, _memcpy_d2d, _np_ptr, _i32p, _u32p, _u64p, _u8p,
                  cigar_batch, finalize_pairs, format_sam, load_library)

_NT4 = np.full(256, 4, np.uint8)
for _i, _c in enumerate(b"ACGT"):
    _NT4[_c] = _i
    _NT4[_c + 32] = _i


def read_ann(prefix: str):
    """contigs [(name, length)] and l_pac from <prefix>.ann (bns_restore, src/bntseq.c:98-160)"""
    with open(prefix + ".ann") as f:
        l_pac, n_seqs, _ = f.readline().split()
        contigs = []
        for _ in range(int(n_seqs)):
            name = f.readline().split()[1]
            _, ln, _ = f.readline().split()
            contigs.append((name, int(ln)))
    return contigs, int(l_pac)


def read_alt(prefix: str, contigs) -> np.ndarray:
    """is_alt per sequence from <prefix>.alt, the reference's way (bns_restore, src/bntseq.c:179-200): the first field of every line
    that does not start with '@' names an ALT contig; names the index does not hold are ignored.  No file: no ALT contigs."""
    alt = np.zeros(len(contigs), np.uint8)
    path = prefix + ".alt"
    if not os.path.exists(path):
        return alt
    where = {}
    for i, c in enumerate(contigs):
        where[c[0]] = i                                   # (kh_put keeps one entry per name; a later duplicate overwrites its value)
    import re
    with open(path, "rb") as f:
        lines = f.read().split(b"\n")
    for k, line in enumerate(lines):
        parts = re.split(rb"[\t\r]", line, maxsplit=1)
        if k == len(lines) - 1 and len(parts) == 1:
            break                                         # (the reference completes a name at a tab, CR or LF: a bare name before EOF is never looked up)
        tok = parts[0].decode("latin-1")
        if tok and tok[0] != "@" and tok in where:
            alt[where[tok]] = 1
    return alt


class ReadSet:
    """reads of a FASTA or FASTQ file as flat arrays: ascii bases back to back + offsets / lengths, names as a NUL-separated blob;
    qual: the qualities at the letters' offsets (FASTQ) or None; comments: (blob, offsets) of the header comments, NUL-separated like
    the names, or None (not kept)"""

    def __init__(self, ascii_, offs, lens, name_blob, name_off, codes=None, qual=None, comments=None):
        self.ascii, self.offs, self.lens, self.name_blob, self.name_off = ascii_, offs, lens, name_blob, name_off
        self.codes = codes                      # nt4 codes of the letters when the loader made them (bmh_reads_load_fasta), else None
        self.qual, self.comments = qual, comments
        self.groups = None                      # bam_to_reads(read_groups=...): every read's index in that list

    def __len__(self):
        return len(self.lens)

    def slice(self, b0: int, b1: int) -> "ReadSet":
        b1 = min(b1, len(self))
        a0 = int(self.offs[b0]); a1 = int(self.offs[b1 - 1] + self.lens[b1 - 1])
        n0 = int(self.name_off[b0]); n1 = int(self.name_off[b1]) if b1 < len(self) else len(self.name_blob)
        cm = None
        if self.comments is not None:
            cb, co = self.comments
            c0 = int(co[b0]); c1 = int(co[b1]) if b1 < len(self) else len(cb)
            cm = (cb[c0:c1], co[b0:b1] - np.uint64(c0))
        return ReadSet(self.ascii[a0:a1], self.offs[b0:b1] - np.uint64(a0), self.lens[b0:b1], self.name_blob[n0:n1], self.name_off[b0:b1] - np.uint64(n0),
                       codes=None if self.codes is None else self.codes[a0:a1], qual=None if self.qual is None else self.qual[a0:a1], comments=cm)

    @classmethod
    def from_lists(cls, names, seqs, quals=None, comments=None) -> "ReadSet":
        """quals: one quality string (str / bytes / uint8 array) per read, of its length; comments: one str per read ("" = none)"""
        seqs = [np.frombuffer(s.encode(), dtype=np.uint8) if isinstance(s, str) else np.asarray(s, dtype=np.uint8) for s in seqs]
        lens = np.array([len(s) for s in seqs], np.uint32)
        offs = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.uint64) if len(seqs) else np.zeros(0, np.uint64)
        ascii_ = np.concatenate(seqs) if len(seqs) and lens.sum() else np.zeros(1, np.uint8)
        enc = [n.encode() + b"\0" for n in names]
        blob = np.frombuffer(b"".join(enc), dtype=np.uint8) if enc else np.zeros(1, np.uint8)
        noff = np.concatenate([[0], np.cumsum([len(e) for e in enc])[:-1]]).astype(np.uint64) if enc else np.zeros(0, np.uint64)
        qual = None
        if quals is not None:
            qs = [np.frombuffer(q.encode() if isinstance(q, str) else bytes(q), dtype=np.uint8) for q in quals]
            if len(qs) != len(seqs) or any(len(q) != len(x) for q, x in zip(qs, seqs)):
                raise ValueError("quals: one quality string of its read's length per read")
            qual = np.concatenate(qs) if len(qs) and lens.sum() else np.zeros(1, np.uint8)
        cm = None
        if comments is not None:
            ce = [c.encode() + b"\0" for c in comments]
            if len(ce) != len(seqs):
                raise ValueError("comments: one per read")
            cm = (np.frombuffer(b"".join(ce), dtype=np.uint8) if ce else np.zeros(1, np.uint8),
                  np.concatenate([[0], np.cumsum([len(e) for e in ce])[:-1]]).astype(np.uint64) if ce else np.zeros(0, np.uint64))
        return cls(ascii_, offs, lens, blob, noff, qual=qual, comments=cm)


def read_fasta_reads(path: str) -> ReadSet:
    """one '>' header line and one sequence line per read (the only layout the reference's seeding library parses,
    src/GPUSeed/seed_gen.cu:1698-1728), through the library's loader (bmh_reads_load_fasta: host threads, letters + nt4 codes)"""
    from .lib import load_fasta_reads
    d = load_fasta_reads(path)
    if len(d["lens"]) == 0:
        return ReadSet.from_lists([], [])
    return ReadSet(d["ascii"], d["offs"], d["lens"], d["names"], d["name_offs"], codes=d["codes"])


def read_reads(path: str, comments: bool = False) -> ReadSet:
    """a FASTA or FASTQ file (the first non-blank byte decides) through the library's loader (bmh_reads_load): read_fasta_reads plus the
    qualities of a FASTQ file and, with comments=True, the header comments (what -C writes).  A malformed file raises ValueError."""
    from .lib import load_reads
    d = load_reads(path, comments=comments)
    if len(d["lens"]) == 0:
        return ReadSet.from_lists([], [], comments=[] if comments else None)
    cm = (d["comments"], d["comment_offs"]) if d["comments"] is not None else None
    return ReadSet(d["ascii"], d["offs"], d["lens"], d["names"], d["name_offs"], codes=d["codes"], qual=d["quals"], comments=cm)


def read_reads_files(path1: str, path2: str | None = None, comments: bool = False, host: bool = False, collate: bool = False, collate_mem=None, keep_rg: bool = False) -> ReadSet:
    """one or two read files of any shape the reference takes (bmh_reads_load_files): FASTA or FASTQ with records over any number of lines, plain, gzip or
    BGZF, regular files or pipes; path2: the mates (read i of each file -> reads 2i, 2i+1).  The records are cut on the device; host=True: by the host
    walker alone (no device needed).  A refused file raises ValueError (lib.ReadFileError); when one file ends before the other, its `partial` attribute
    is the ReadSet of the complete pairs.
    collate=True: `path1` is a paired BAM in any record order, a coordinate-sorted one for instance -- the mates of a pair are found by name, and the reads are
    the pairs in the order in which their later record comes (include/bwamem_hip.h has the definition); text input is refused, a record whose partner never comes
    is refused with the complete pairs in `partial`, and beyond collate_mem bytes of records that wait for their partners (8 GiB by default) the file is refused.
    keep_rg=True: `path1` is a BAM read under its own read groups, as align_files(keep_rg=True) reads it -- the ReadSet's `groups` is the index of every read's
    @RG line in the header, and the refusals are those of that run."""
    from .lib import ReadFileError, load_reads_files

    def wrap(d):
        if len(d["lens"]) == 0:
            return ReadSet.from_lists([], [], comments=[] if comments else None)
        cm = (d["comments"], d["comment_offs"]) if d["comments"] is not None else None
        rs = ReadSet(d["ascii"], d["offs"], d["lens"], d["names"], d["name_offs"], codes=d["codes"], qual=d["quals"], comments=cm)
        if keep_rg:
            rs.groups = d["groups"]
        return rs
    try:
        return wrap(load_reads_files(path1, path2, comments=comments, host=host, collate=collate, collate_mem=collate_mem, keep_rg=keep_rg))
    except ReadFileError as e:
        if getattr(e, "partial", None) is not None:
            e.partial = wrap(e.partial)
        raise


def bam_to_reads(records: bytes, comments: bool = False, host: bool = False, read_groups=None, collate: bool = False, collate_mem=None) -> ReadSet:
    """uncompressed BAM records (without the header) as the reads read_reads_files gives for the BAM file that holds them (bmh_bam_reads_device; host=True:
    bmh_bam_reads_host, no device needed): `samtools fastq`'s rules -- secondary and supplementary records skipped, reverse-strand records turned back, pairs
    (flag 0x1) as reads 2i / 2i+1, and with comments=True the tags as the comment -C copies.  Refused records raise ValueError (lib.ReadFileError).
    read_groups: a list of read group IDs -- the ReadSet's `groups` is then the index of every read's RG:Z value in that list (whole IDs compared); a kept
    record without an RG tag, with one of another type than Z or with an ID that is not listed, and a pair whose two records name different groups are refused
    naming the record's index.  Records skipped by their flag are not looked at.
    collate=True: the records are in any order and mates are found by name, as read_reads_files(collate=True) finds them (collate_mem: its cap)."""
    from .lib import ReadFileError, bam_reads

    def wrap(d):
        if len(d["lens"]) == 0:
            rs = ReadSet.from_lists([], [], comments=[] if comments else None)
            rs.groups = np.zeros(0, np.uint32) if read_groups is not None else None
            return rs
        cm = (d["comments"], d["comment_offs"]) if d["comments"] is not None else None
        rs = ReadSet(d["ascii"], d["offs"], d["lens"], d["names"], d["name_offs"], codes=d["codes"], qual=d["quals"], comments=cm)
        rs.groups = d["groups"] if read_groups is not None else None
        return rs
    try:
        return wrap(bam_reads(records, comments=comments, host=host, read_groups=read_groups, collate=collate, collate_mem=collate_mem))
    except ReadFileError as e:
        if getattr(e, "partial", None) is not None:
            e.partial = wrap(e.partial)
        raise


def _holds_bam(path) -> bool | None:
    """does a regular file hold a BAM (a BGZF member whose text begins with the magic bytes)?  None for what cannot be looked at without taking its bytes (a pipe)"""
    import zlib
    try:
        if not os.path.isfile(path) or os.path.getsize(path) == 0:      # (an empty file is the library's to name)
            return None
        with open(path, "rb") as f:
            head = f.read(1 << 16)
        return zlib.decompressobj(31).decompress(head, 4)[:4] == b"BAM\1"
    except (OSError, zlib.error):
        return False


def bam_read_groups(header_text, markdup: bool = False) -> list:
    """the read groups of a BAM header's text (str or bytes): [(the @RG line verbatim, its ID, its library), ...] in file order -- the library by rg_library's
    rules.  The text ends at its first NUL, the last line may lack its newline, a CR before the newline is dropped, other lines are ignored.  Raises ValueError
    naming the line: no @RG line, a line without a non-empty ID of at most 255 bytes or whose fields are not tab-separated XX:value, a repeated ID, more than
    65535 groups; with markdup=True also more than 255 distinct libraries."""
    from .lib import bam_header_read_groups
    lines, _lib = bam_header_read_groups(header_text, markdup=markdup)
    return [(ln, next(f[3:] for f in ln.split("\t")[1:] if f.startswith("ID:")), rg_library(ln)) for ln in lines]


def read_fasta_reads_numpy(path: str) -> ReadSet:
    """the same parse with numpy array operations (what read_fasta_reads was before the library had a loader; kept as its cross-check)"""
    buf = np.fromfile(path, dtype=np.uint8)
    if buf.size == 0:
        return ReadSet.from_lists([], [])
    if buf[-1] != 10:
        buf = np.concatenate([buf, np.array([10], np.uint8)])
    nl = np.flatnonzero(buf == 10)
    starts = np.concatenate([[0], nl[:-1] + 1]); ends = nl.copy()
    cr = (ends > starts) & (buf[np.maximum(ends - 1, 0)] == 13)
    ends = ends - cr
    keep = ends > starts
    starts, ends = starts[keep], ends[keep]
    is_hdr = buf[starts] == ord(">")
    if (~is_hdr).sum() != is_hdr.sum() or not is_hdr[0::2].all() or is_hdr[1::2].any():
        raise ValueError("reads file: expected alternating '>' header and sequence lines")
    hs, he = starts[0::2] + 1, ends[0::2]
    ss, se = starts[1::2], ends[1::2]
    lens = (se - ss).astype(np.uint32)
    offs = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.uint64)
    # gather the sequence bytes (drop headers / newlines): a mask over the buffer
    mark = np.zeros(buf.size + 1, np.int8); np.add.at(mark, ss, 1); np.add.at(mark, se, -1)
    ascii_ = buf[np.cumsum(mark[:-1]) > 0]
    # names: header up to the first blank, NUL-terminated in place
    hb = buf.copy()
    blank = (hb == 32) | (hb == 9)
    first_blank = np.full(len(hs), -1, np.int64)
    bl = np.flatnonzero(blank)
    if bl.size:
        j = np.searchsorted(bl, hs)
        ok = (j < bl.size)
        cand = np.where(ok, bl[np.minimum(j, bl.size - 1)], -1)
        first_blank = np.where(ok & (cand < he), cand, -1)
    name_end = np.where(first_blank >= 0, first_blank, he)
    nlen = (name_end - hs).astype(np.int64)
    # a trailing "/<digit>" is not part of the name (trim_readno, src/bwa.c:27-31)
    e1, e2 = buf[np.maximum(name_end - 1, 0)], buf[np.maximum(name_end - 2, 0)]
    trim = (nlen > 2) & (e2 == ord("/")) & (e1 >= ord("0")) & (e1 <= ord("9"))
    name_end = name_end - 2 * trim
    nlen = (name_end - hs).astype(np.int64)
    noff = np.concatenate([[0], np.cumsum(nlen + 1)[:-1]]).astype(np.uint64)
    blob = np.zeros(int((nlen + 1).sum()), np.uint8)
    nmark = np.zeros(buf.size + 1, np.int8); np.add.at(nmark, hs, 1); np.add.at(nmark, name_end, -1)
    src = np.flatnonzero(np.cumsum(nmark[:-1]) > 0)
    dst = np.arange(src.size) + np.repeat(np.arange(len(hs)), nlen)          # one NUL after every name
    blob[dst] = buf[src]
    return ReadSet(ascii_ if ascii_.size else np.zeros(1, np.uint8), offs, lens, blob, noff)


def _raise_beyond_cap(e: Exception) -> None:
    """a batch refused because a query side exceeds the extension cap (768 bases by default; EXT_LONG_MAX with long_reads) -> NotImplementedError"""
    msg = str(e)
    if "extension cap" in msg:
        raise NotImplementedError(msg + ": reads this long are beyond the extension kernels of this aligner (Aligner(long_reads=True) takes "
                                  "flanks of up to EXT_LONG_MAX bases; the reference's own GASAL2 build is sized by MAX_SEQ_LEN, README.md:38)") from e


def parse_rg_line(v: str, what: str = "-R"):
    """a read group line as the command line gives it -> (the line, its ID) by bwa_set_rg's rules (src/bwa.c:425-452); `what` names the option in messages.
    bwa_escape (src/bwa.c:409-423): ONE pass from the left -- a backslash consumes the character behind it, which becomes a tab / newline / carriage return /
    backslash for t / n / r / \\ and nothing at all otherwise ("\\\\t" is a backslash and a 't', not a backslash and a tab)"""
    import re
    if not v.startswith("@RG"):
        raise ValueError(f"{what}: the read group line must start with @RG")
    line = re.sub(r"\\(.?)", lambda m: {"t": "\t", "n": "\n", "r": "\r", "\\": "\\"}.get(m.group(1), ""), v, flags=re.S)
    if "\tID:" not in line:
        raise ValueError(f"{what}: the read group line must hold an ID")
    rid = re.split("[\t\n]", line.split("\tID:", 1)[1], 1)[0]            # the ID ends at the first tab or newline (src/bwa.c:440-446)
    if len(rid) > 255:
        raise ValueError(f"{what}: @RG:ID is longer than 255 characters")
    return line, rid


def rg_library(rg_line: str) -> str:
    """the library of a read group line: its LB field, else Picard's Unknown Library"""
    lib = "Unknown Library"
    for f in rg_line.split("\t")[1:]:
        if f.startswith("LB:") and len(f) > 3:
            lib = f[3:]
    return lib


_METRICS_COLUMNS = ("LIBRARY", "UNPAIRED_READS_EXAMINED", "READ_PAIRS_EXAMINED", "SECONDARY_OR_SUPPLEMENTARY_RDS", "UNMAPPED_READS", "UNPAIRED_READ_DUPLICATES", "READ_PAIR_DUPLICATES",
                    "PERCENT_DUPLICATION")


# with optical duplicates counted: Picard's column order, the two columns that need them included
_METRICS_COLUMNS_OPTICAL = _METRICS_COLUMNS[:-1] + ("READ_PAIR_OPTICAL_DUPLICATES", "PERCENT_DUPLICATION", "ESTIMATED_LIBRARY_SIZE")


def _metrics_row(lib: str, counts: dict) -> list:
    fr, pr, df, dp = counts["fragments_examined"], counts["pairs_examined"], counts["duplicate_fragments"], counts["duplicate_pairs"]
    den = fr + 2 * pr
    row = [lib, fr, pr, counts["secondary_or_supplementary"], counts["unmapped_records"], df, dp, "%.6f" % ((df + 2 * dp) / den) if den else "0"]
    if "optical_duplicate_pairs" in counts:                       # (counts of a run with an optical distance)
        from .lib import estimate_library_size
        od = counts["optical_duplicate_pairs"]
        size = estimate_library_size(pr - od, pr - dp)
        row = row[:-1] + [od, row[-1], "" if size is None else size]
    return row


def markdup_metrics_text_libraries(library_counts: dict) -> str:
    """markdup_metrics_text for a run over read groups: the class line, the header row and one row per library -- library_counts: {library name: counts}, in order
    of first appearance (dicts keep it)"""
    cols = _METRICS_COLUMNS_OPTICAL if any("optical_duplicate_pairs" in c for c in library_counts.values()) else _METRICS_COLUMNS
    return "## METRICS CLASS\tbwamem_hip.DuplicationMetrics\n" + "\t".join(cols) + "\n" + \
           "".join("\t".join(str(v) for v in _metrics_row(lib, c)) + "\n" for lib, c in library_counts.items())


def markdup_metrics_text(counts: dict, rg_line: str = "") -> str:
    """the Picard-style metrics table of a marked run: a class line, the header row and one row (one library per run: the read group's LB, else Unknown Library).
    Counts that hold "optical_duplicate_pairs" (a run with optical_distance) give Picard's full column order: READ_PAIR_OPTICAL_DUPLICATES before
    PERCENT_DUPLICATION and ESTIMATED_LIBRARY_SIZE (empty where Picard leaves it empty) behind it; so with markdup_metrics_text_libraries"""
    lib = "Unknown Library"
    for f in rg_line.split("\t")[1:]:
        if f.startswith("LB:") and len(f) > 3:
            lib = f[3:]
    if "optical_duplicate_pairs" in counts:
        return "## METRICS CLASS\tbwamem_hip.DuplicationMetrics\n" + "\t".join(_METRICS_COLUMNS_OPTICAL) + "\n" + "\t".join(str(v) for v in _metrics_row(lib, counts)) + "\n"
    fr, pr, df, dp = counts["fragments_examined"], counts["pairs_examined"], counts["duplicate_fragments"], counts["duplicate_pairs"]
    den = fr + 2 * pr
    cols = [("LIBRARY", lib), ("UNPAIRED_READS_EXAMINED", fr), ("READ_PAIRS_EXAMINED", pr), ("SECONDARY_OR_SUPPLEMENTARY_RDS", counts["secondary_or_supplementary"]),
            ("UNMAPPED_READS", counts["unmapped_records"]), ("UNPAIRED_READ_DUPLICATES", df), ("READ_PAIR_DUPLICATES", dp),
            ("PERCENT_DUPLICATION", "%.6f" % ((df + 2 * dp) / den) if den else "0")]
    return "## METRICS CLASS\tbwamem_hip.DuplicationMetrics\n" + "\t".join(c for c, _v in cols) + "\n" + "\t".join(str(v) for _c, v in cols) + "\n"


COVERAGE_TABLE_HEADER = "#rname\tstartpos\tendpos\tnumreads\tcovbases\tcoverage\tmeandepth\tmaxdepth\tmeanmapq"


def coverage_table_text(cov: dict, contigs) -> str:
    """the table of `samtools coverage`: a header line, one row per contig in header order and a last row `total` -- name, 1, length, counted reads, covered
    bases, their percentage, mean depth, largest depth, mean mapq (the three with %.6g; a mean is 0 where its divisor is 0)"""
    def row(name, length, reads, covb, sumd, maxd, mapq):
        return "%s\t1\t%d\t%d\t%d\t%.6g\t%.6g\t%d\t%.6g" % (name, length, reads, covb, 100.0 * covb / length if length else 0.0, sumd / length if length else 0.0, maxd,
                                                         mapq / reads if reads else 0.0)
    lines = [COVERAGE_TABLE_HEADER]
    for c, (name, length) in enumerate(contigs):
        lines.append(row(name, int(length), int(cov["n_reads"][c]), int(cov["cov_bases"][c]), int(cov["sum_depth"][c]), int(cov["max_depth"][c]), int(cov["sum_mapq"][c])))
    tot = {k: int(sum(int(v) for v in cov[k])) for k in ("n_reads", "cov_bases", "sum_depth", "sum_mapq")}
    lines.append(row("total", sum(int(l) for _n, l in contigs), tot["n_reads"], tot["cov_bases"], tot["sum_depth"], max([int(v) for v in cov["max_depth"]] or [0]), tot["sum_mapq"]))
    return "\n".join(lines) + "\n"


def coverage_hist_text(cov: dict) -> str:
    """depth, bases, fraction_at_or_above (%.6f): 1001 rows, the last labelled 1000+"""
    hist = [int(v) for v in cov["hist"]]
    total, lines, above = sum(hist), ["depth\tbases\tfraction_at_or_above"], sum(hist)
    for d, h in enumerate(hist):
        lines.append("%s\t%d\t%.6f" % ("1000+" if d == len(hist) - 1 else str(d), h, above / total if total else 0.0))
        above -= h
    return "\n".join(lines) + "\n"


def coverage_bed_text(cov: dict, contigs, bin: int) -> str:
    """name, start, end, mean depth (%.2f): one row per bin of `bin` positions, empty ones too, a contig's last bin ending at its length"""
    lines, k = [], 0
    for name, length in contigs:
        for a in range(0, int(length), bin):
            b = min(a + bin, int(length))
            lines.append("%s\t%d\t%d\t%.2f" % (name, a, b, int(cov["bin_sum"][k]) / (b - a)))
            k += 1
    assert k == len(cov["bin_sum"])
    return "".join(l + "\n" for l in lines)


COVERAGE_KEYWORDS = ("coverage", "coverage_hist", "coverage_bed", "coverage_bin", "coverage_min_mapq", "coverage_deletions")


def _coverage_keywords(f):
    """align_file / align_files / align_groups: the outermost call's coverage keywords are checked (coverage_request, with the call's `sort`) and kept in
    self._cov_req for as long as the run; the calls the method makes on its way (they hand no coverage keyword on) find the request there"""
    sig = inspect.signature(f)

    @functools.wraps(f)
    def call(self, *args, **kw):
        if getattr(self, "_cov_req", None) is not None:
            return f(self, *args, **kw)
        given = sig.bind(self, *args, **kw)
        given.apply_defaults()
        req = coverage_request(f.__name__, given.arguments["sort"], *(given.arguments[k] for k in COVERAGE_KEYWORDS))
        if req is None:
            return f(self, *args, **kw)
        self._cov_req = req
        try:
            return f(self, *args, **kw)
        finally:
            self._cov_req = None
    return call


def coverage_request(what: str, sort: bool, coverage=None, coverage_hist=None, coverage_bed=None, coverage_bin=None, coverage_min_mapq=None, coverage_deletions=False):
    """the coverage keywords of align_file / align_files / align_groups, checked -> None (none given) or a dict of them; ValueError otherwise"""
    outs = coverage is not None or coverage_hist is not None or coverage_bed is not None
    mods = coverage_bin is not None or coverage_min_mapq is not None or bool(coverage_deletions)
    if not outs and not mods:
        return None
    if not sort:
        raise ValueError(f"{what}: the coverage options need sort=True: depth is computed where the sorted file is written")
    if (coverage_bed is None) != (coverage_bin is None):
        raise ValueError(f"{what}: coverage_bed and coverage_bin go together (the bins of the BED file)")
    if not outs:
        raise ValueError(f"{what}: coverage_min_mapq and coverage_deletions need coverage, coverage_hist or coverage_bed (they say what is counted, not where it goes)")
    for nm, v, lo, hi in (("coverage_bin", coverage_bin, 1, 0xffffffff), ("coverage_min_mapq", coverage_min_mapq, 0, 255)):
        if v is not None and (not isinstance(v, (int, np.integer)) or isinstance(v, bool) or not lo <= v <= hi):
            raise ValueError(f"{what}: {nm} {v!r}: an integer in {lo} .. {hi}")
    return dict(table=coverage, hist=coverage_hist, bed=coverage_bed, bin=int(coverage_bin or 0), min_mapq=int(coverage_min_mapq or 0), deletions=bool(coverage_deletions))


STATS_KEYWORDS = ("flagstat", "idxstats", "stats", "insert_cap")


def stats_request(what: str, sort: bool, flagstat=None, idxstats=None, stats=None, insert_cap=None):
    """the statistics keywords of align_file / align_files / align_groups / bam_post_file, checked -> None (none given) or a dict of them; ValueError otherwise"""
    outs = flagstat is not None or idxstats is not None or stats is not None
    if not outs and insert_cap is None:
        return None
    if not sort:
        raise ValueError(f"{what}: flagstat, idxstats, stats and insert_cap need sort=True: the statistics are computed where the sorted file is written")
    if not outs:
        raise ValueError(f"{what}: insert_cap needs flagstat, idxstats or stats (it says how the insert sizes are binned, not where they go)")
    if insert_cap is not None and (not isinstance(insert_cap, (int, np.integer)) or isinstance(insert_cap, bool) or not 2 <= insert_cap <= 65536):
        raise ValueError(f"{what}: insert_cap {insert_cap!r}: an integer in 2 .. 65536")
    return dict(flagstat=flagstat, idxstats=idxstats, stats=stats, insert_cap=int(insert_cap or 65536))


def _stats_keywords(f):
    """_coverage_keywords for the statistics keywords: the outermost call's request stays in self._stats_req for as long as the run"""
    sig = inspect.signature(f)

    @functools.wraps(f)
    def call(self, *args, **kw):
        if getattr(self, "_stats_req", None) is not None:
            return f(self, *args, **kw)
        given = sig.bind(self, *args, **kw)
        given.apply_defaults()
        req = stats_request(f.__name__, given.arguments["sort"], *(given.arguments[k] for k in STATS_KEYWORDS))
        if req is None:
            return f(self, *args, **kw)
        self._stats_req = req
        try:
            return f(self, *args, **kw)
        finally:
            self._stats_req = None
    return call


RECAL_KEYWORDS = ("recal", "known_sites", "recal_min_qual", "recal_max_cycle", "apply_recal", "apply_recal_report")


def recal_request(what: str, sort: bool, recal=None, known_sites=None, recal_min_qual=None, recal_max_cycle=None, apply_recal=None, apply_recal_report=None, need: str = "sort=True", sorted_out: bool = True):
    """the recalibration keywords of align_file / align_files / align_groups / bam_post_file, checked -> None (none given) or a dict of them; ValueError otherwise.
    apply_recal (a path or read_recal_table's dict): the table applied to the qualities as they are written -- read here, so that a file that is
    no table is refused before anything is written; "table" is None where no table is counted.  sort: what `need` asks for, which counting needs; sorted_out: a
    sorted file is written, which applying needs"""
    sites = [known_sites] if isinstance(known_sites, (str, bytes, os.PathLike)) else list(known_sites or [])
    if apply_recal is None and apply_recal_report is not None:
        raise ValueError(f"{what}: apply_recal_report needs apply_recal (it says what the applied table changed)")
    if recal is None:
        if sites or recal_min_qual is not None or recal_max_cycle is not None:
            raise ValueError(f"{what}: known_sites, recal_min_qual and recal_max_cycle need recal (they say what is counted, not where it goes)")
        if apply_recal is None:
            return None
    elif not sort:
        raise ValueError(f"{what}: the recalibration options need {need}: the table is counted where the sorted file is written")
    table = None
    if apply_recal is not None:
        if not sorted_out:
            raise ValueError(f"{what}: apply_recal needs sort=True: the qualities are rewritten where the sorted file is written")
        if isinstance(recal, (str, os.PathLike)) and isinstance(apply_recal, (str, os.PathLike)) and os.path.abspath(os.fspath(recal)) == os.path.abspath(os.fspath(apply_recal)):
            raise ValueError(f"{what}: recal and apply_recal name the same file: counting and applying one table in one run would take two passes over the windows")
        from .recal import read_recal_table
        table = read_recal_table(os.fspath(apply_recal)) if isinstance(apply_recal, (str, os.PathLike)) else apply_recal
        if not isinstance(table, dict) or "cycle_m" not in table or "context_m" not in table:
            raise ValueError(f"{what}: apply_recal takes a path or read_recal_table's dict")
    for nm, v, lo, hi in (("recal_min_qual", recal_min_qual, 0, 93), ("recal_max_cycle", recal_max_cycle, 1, 65535)):
        if v is not None and (not isinstance(v, (int, np.integer)) or isinstance(v, bool) or not lo <= v <= hi):
            raise ValueError(f"{what}: {nm} {v!r}: an integer in {lo} .. {hi}")
    return dict(table=recal, known_sites=[os.fspath(p) for p in sites], min_qual=6 if recal_min_qual is None else int(recal_min_qual), max_cycle=500 if recal_max_cycle is None else int(recal_max_cycle),
                apply=table, apply_report=apply_recal_report)


def _recal_keywords(f):
    """_coverage_keywords for the recalibration keywords: the outermost call's request stays in self._recal_req for as long as the run"""
    sig = inspect.signature(f)

    @functools.wraps(f)
    def call(self, *args, **kw):
        if getattr(self, "_recal_req", None) is not None:
            return f(self, *args, **kw)
        given = sig.bind(self, *args, **kw)
        given.apply_defaults()
        req = recal_request(f.__name__, given.arguments["sort"], *(given.arguments[k] for k in RECAL_KEYWORDS), sorted_out=given.arguments["sort"])
        if req is None:
            return f(self, *args, **kw)
        if given.arguments.get("keep_rg") and req["table"] is not None:                        # the table's read groups are the input's: its header is read here, ahead of the run
            from .bam import peek_header
            src = given.arguments["reads"]
            if not isinstance(src, (str, os.PathLike)) or not os.path.isfile(src):
                raise ValueError(f"{f.__name__}: recal with keep_rg=True reads the input's header before the run: a BAM file, not a pipe")
            text, _contigs = peek_header(os.fspath(src))
            req["groups"] = [g[1] for g in bam_read_groups(text)]
            if len(req["groups"]) > 255:
                raise ValueError(f"{f.__name__}: {len(req['groups'])} read groups: the recalibration table holds at most 255")
        self._recal_req = req
        try:
            return f(self, *args, **kw)
        finally:
            self._recal_req = None
    return call


def read_amb(prefix: str) -> list:
    """the reference's holes from <prefix>.amb as (offset, length) pairs in pac; no file: none"""
    try:
        with open(prefix + ".amb") as f:
            f.readline()
            return [(int(a), int(b)) for a, b, *_ in (ln.split() for ln in f if ln.strip())]
    except FileNotFoundError:
        return []


def _pct(a: int, b: int) -> str:
    return "%.2f%%" % (100.0 * a / b) if b else "N/A"


def flagstat_text(st: dict) -> str:
    """`samtools flagstat`'s sixteen lines, in its order and wording, from bam_stats' "flag" (QC-passed + QC-failed); a percentage over 0 reads N/A"""
    p, f = ([int(v) for v in row] for row in st["flag"])
    (total, primary, secondary, supp, dup, pdup, mapped, pmapped, paired, read1, read2, proper, both, single, diff, diff5) = range(16)
    def line(k, words, over=None):
        tail = "" if over is None else " (%s : %s)" % (_pct(p[k], p[over]), _pct(f[k], f[over]))
        return "%d + %d %s%s" % (p[k], f[k], words, tail)
    return "\n".join([line(total, "in total (QC-passed reads + QC-failed reads)"), line(primary, "primary"), line(secondary, "secondary"), line(supp, "supplementary"),
                      line(dup, "duplicates"), line(pdup, "primary duplicates"), line(mapped, "mapped", total), line(pmapped, "primary mapped", primary),
                      line(paired, "paired in sequencing"), line(read1, "read1"), line(read2, "read2"), line(proper, "properly paired", paired),
                      line(both, "with itself and mate mapped"), line(single, "singletons", paired), line(diff, "with mate mapped to a different chr"),
                      line(diff5, "with mate mapped to a different chr (mapQ>=5)")]) + "\n"


def idxstats_text(st: dict, contigs) -> str:
    """`samtools idxstats`: name, length, mapped, unmapped per contig in header order, then the row of the records without a contig"""
    rows = ["%s\t%d\t%d\t%d" % (name, int(length), int(st["contig_mapped"][c]), int(st["contig_unmapped"][c])) for c, (name, length) in enumerate(contigs)]
    rows.append("*\t0\t0\t%d" % int(st["unplaced"][0]))
    return "".join(r + "\n" for r in rows)


def _hist_median(values, counts):
    """the median of the values (ascending) with their counts: the mean of the two middle ones when their number is even"""
    cum = np.cumsum(counts)
    n = int(cum[-1])
    lo, hi = values[int(np.searchsorted(cum, (n - 1) // 2 + 1))], values[int(np.searchsorted(cum, n // 2 + 1))]
    return (float(lo) + float(hi)) / 2


def insert_size_metrics(hist, smallest, largest) -> dict:
    """the insert sizes of one orientation -- hist [cap + 1] (index s: the pairs of size s; the last bin: every size from cap up, taken as cap), the exact smallest
    and largest size -- -> pairs, median, mad (the median of |x - median|), mode (the smallest size with the largest count), min, max, mean and sd over the
    sizes <= min(median + 10 * mad, cap - 1) (Picard's trim of the tail; sd with n - 1, 0 for one value).  Medians of an even number of values are the mean of
    the two middle ones.  No pair: every value 0."""
    h = np.asarray(hist, dtype=np.uint64)
    cap = len(h) - 1
    at = [int(s) for s in np.flatnonzero(h)]
    cnt = [int(h[s]) for s in at]
    pairs = sum(cnt)
    if not pairs:
        return dict(pairs=0, median=0.0, mad=0.0, mode=0, min=0, max=0, mean=0.0, sd=0.0)
    median = _hist_median(at, cnt)
    dev = sorted((abs(s - median), c) for s, c in zip(at, cnt))
    mad = _hist_median([d for d, _c in dev], [c for _d, c in dev])
    mode = at[int(np.argmax(cnt))]
    limit = min(median + 10 * mad, cap - 1)
    kept = [(s, c) for s, c in zip(at, cnt) if s <= limit]
    n = sum(c for _s, c in kept)
    mean = sum(s * c for s, c in kept) / n if n else 0.0
    sd = (sum(c * (s - mean) ** 2 for s, c in kept) / (n - 1)) ** 0.5 if n > 1 else 0.0
    return dict(pairs=pairs, median=median, mad=mad, mode=int(mode), min=int(smallest), max=int(largest), mean=float(mean), sd=float(sd))


def stats_text(st: dict, contigs) -> str:
    """one tab-separated text, every line under a section key: FS name passed failed (the flag counts), IX name length mapped unmapped (the contigs, then *),
    SN name value (the summary words and error_rate = edit_distance / bases_aligned, %.6e; 0 over no base), MQ mapq count (the bins that hold a read), IS size FR
    RF TANDEM (the sizes that hold a pair; the overflow row is labelled `cap+`), IM orientation pairs median MAD mode min max mean SD (%.1f %.1f, then %.2f %.2f;
    the orientations that hold a pair)"""
    from .lib import BAM_STATS_FLAGS, BAM_STATS_ORIENTATIONS, BAM_STATS_SUMMARY
    rows = ["FS\t%s\t%d\t%d" % (nm, int(st["flag"][0][k]), int(st["flag"][1][k])) for k, nm in enumerate(BAM_STATS_FLAGS)]
    rows += ["IX\t" + l for l in idxstats_text(st, contigs).split("\n")[:-1]]
    s = {nm: int(st["summary"][k]) for k, nm in enumerate(BAM_STATS_SUMMARY)}
    rows += ["SN\t%s\t%d" % (nm, s[nm]) for nm in BAM_STATS_SUMMARY]
    rows.append("SN\terror_rate\t%s" % ("%.6e" % (s["edit_distance"] / s["bases_aligned"]) if s["bases_aligned"] else "0"))
    rows += ["MQ\t%d\t%d" % (q, int(v)) for q, v in enumerate(st["mapq"]) if int(v)]
    h = st["insert_hist"]
    cap = h.shape[1] - 1
    for size in np.flatnonzero(h.any(axis=0)):
        rows.append("IS\t%s\t%d\t%d\t%d" % ("%d+" % cap if size == cap else str(int(size)), int(h[0][size]), int(h[1][size]), int(h[2][size])))
    for o, nm in enumerate(BAM_STATS_ORIENTATIONS):
        m = insert_size_metrics(h[o], st["insert_min"][o], st["insert_max"][o])
        if m["pairs"]:
            rows.append("IM\t%s\t%d\t%.1f\t%.1f\t%d\t%d\t%d\t%.2f\t%.2f" % (nm, m["pairs"], m["median"], m["mad"], m["mode"], m["min"], m["max"], m["mean"], m["sd"]))
    return "".join(r + "\n" for r in rows)


def write_flagstat(st: dict, dst) -> None:
    """flagstat_text of bam_stats' dict to dst: a path or a text file object"""
    _write_text(dst, flagstat_text(st))


def write_idxstats(st: dict, contigs, dst) -> None:
    """idxstats_text to dst: a path or a text file object"""
    _write_text(dst, idxstats_text(st, contigs))


def write_stats(st: dict, contigs, dst) -> None:
    """stats_text to dst: a path or a text file object"""
    _write_text(dst, stats_text(st, contigs))


def write_stats_texts(req: dict, st: dict, contigs) -> None:
    """the texts a statistics request asks for, to their paths or file objects"""
    if req["flagstat"] is not None:
        write_flagstat(st, req["flagstat"])
    if req["idxstats"] is not None:
        write_idxstats(st, contigs, req["idxstats"])
    if req["stats"] is not None:
        write_stats(st, contigs, req["stats"])


def _write_text(dst, text: str) -> None:
    if hasattr(dst, "write"):
        dst.write(text)
    else:
        with open(dst, "w") as f:
            f.write(text)


class Aligner:
    def __init__(self, prefix: str | None, device: str = "cuda:0", n_threads: int = 0, _mem=None, sa_intv: int | None = 1,
                 long_reads: bool = False):
        # long_reads: the extension cap of the chain workspace and of the native aligner is EXT_LONG_MAX -- extension flanks of
        # 769 .. EXT_LONG_MAX bases go to the long-query kernel instead of raising; batches without such a flank take the same path either way
        self.long_reads = bool(long_reads)
        self.L = load_library()
        self.dev = torch.device(device)
        self.prefix = prefix                                  # (the recalibration table reads the reference's holes from <prefix>.amb)
        if _mem is not None:                                  # (index, contigs, packed reference) already in memory: from_memory()
            idx, self.contigs, self.pac = _mem
            self.l_pac = sum(c[1] for c in self.contigs)
            self.alt = np.ascontiguousarray([1 if (len(c) > 2 and c[2]) else 0 for c in self.contigs], dtype=np.uint8)
            self.contigs = [(c[0], c[1]) for c in self.contigs]
        else:
            idx = fmindex.read_index(prefix)
            self.contigs, self.l_pac = read_ann(prefix)
            self.alt = read_alt(prefix, self.contigs)
            pac = np.fromfile(prefix + ".pac", dtype=np.uint8)
            self.pac = np.ascontiguousarray(np.concatenate([pac[: (self.l_pac + 3) // 4], np.zeros(2, np.uint8)]))
        self.index = Index.upload(idx, pac=self.pac, l_pac=self.l_pac)
        if sa_intv:                                            # denser suffix-array samples than the files hold (every 16th row): ms on the device
            self.index.densify_sa(sa_intv)
        self.copt = ChainOpt(); self.L.bmh_chain_opt_default(C.byref(self.copt))
        self.ep = ExtParams.default()
        self.po = PostOpt(); self.L.bmh_post_opt_default(C.byref(self.po))
        self.pe = PeOpt(); self.L.bmh_pe_opt_default(C.byref(self.pe))
        self.reseed = ReseedOpt.default()                        # BWA-MEM's second and third seeding rounds: off until -g
        # ALT contigs (<prefix>.alt): the chain filter, the marking of primary hits, MAPQ, the XA / pa tags and the clipping depend on them
        # (src/bwamem.c:446,518,571-574,702,714-760,1540,1663,1742,1755); the region tail of such an index runs on the host
        self.has_alt = bool(self.alt.any())
        if self.has_alt:
            self.copt.contig_is_alt = self.alt.ctypes.data; self.po.contig_is_alt = self.alt.ctypes.data
        self.n_threads = n_threads or int(self.L.bmh_effective_cpus())          # (the CPUs this process is granted, not the ones the machine shows)
        self.profile = bool(os.environ.get("BMH_ALIGNER_PROFILE"))
        self.c_off = np.ascontiguousarray(np.concatenate([[0], np.cumsum([c[1] for c in self.contigs])]), dtype=np.int64)

    @classmethod
    def from_memory(cls, idx, genome_fwd: np.ndarray, contigs=None, **kw) -> "Aligner":
        """idx: fmindex.FMDIndex of genome_fwd (nt4 codes); contigs: [(name, length)], default one sequence chrS"""
        pad = (-len(genome_fwd)) % 4
        codes = np.concatenate([genome_fwd, np.zeros(pad, np.uint8)]).reshape(-1, 4)
        pac = ((codes[:, 0] << 6) | (codes[:, 1] << 4) | (codes[:, 2] << 2) | codes[:, 3]).astype(np.uint8)
        pac = np.ascontiguousarray(np.concatenate([pac, np.zeros(2, np.uint8)]))
        return cls(None, _mem=(idx, contigs or [("chrS", int(len(genome_fwd)))], pac), **kw)

    def set_options(self, argv, *, split_factor: float | None = None, split_width: int | None = None, max_mem_intv: int | None = None) -> None:
        """gase_aln's command-line options (src/fastmap.c:166-262) that reach this path, as a list of strings, e.g.
        ["-k", "23", "-A", "2", "-a"].  The device extension takes -A -B and the DELETION penalties -O -E for both gap
        kinds, as the reference's GPU extension does (src/fastmap.c:417-424); -O/-E given as "del,ins" keep the pair for
        the host stages.  Unlike the reference (update_a, src/fastmap.c), nothing is rescaled by -A: pass every value you want
        changed (-B -O -E -T -U).
        -d and -L are accepted and ignored (they do not reach the reference's GPU extension either).  -C appends every read's header
        comment to its records.  -g turns on BWA-MEM's re-seeding (the second and third seeding rounds of mem_collect_intv); its parameters
        are the keyword arguments split_factor (-r, 1.5), split_width (-s, 10) and max_mem_intv (-y, 20; 0 leaves out the third round).
        Not modelled: -x -r -s -y on the option list (seeding variants the GPU seeding of the reference ignores too), -I -H -V."""
        import math
        co, ep, po, pe = self.copt, self.ep, self.po, self.pe
        i = 0
        def pair(v):
            a, _, b = v.replace(";", ",").partition(",")
            return int(a), int(b) if b else int(a)
        while i < len(argv):
            f = argv[i]
            if f in ("-a", "-M", "-Y", "-S", "-P", "-j", "-C", "-g"):
                if f == "-j":                             # the .alt file is ignored (src/fastmap.c:186,390-392): every sequence belongs to the primary assembly
                    self.alt[:] = 0; self.has_alt = False; co.contig_is_alt = None; po.contig_is_alt = None
                    if getattr(self, "_native", None) is not None: self._native.free(); self._native = None
                    c = getattr(self, "_cw_cache", None)         # a cached chain workspace still holds the ALT table (set_alt): the batch-by-batch path must not filter chains with it
                    if c is not None: c[0].free(); self._cw_cache = None
                elif f == "-a": po.flag_all = 1
                elif f == "-M": po.no_multi = 1
                elif f == "-Y": po.softclip = 1
                elif f == "-C": po.copy_comment = 1
                elif f == "-g": self.reseed.enable = 1              # takes no value (src/fastmap.c:202)
                elif f == "-S": pe.no_rescue = 1
                else: pe.no_pairing = 1
                i += 1; continue
            if i + 1 >= len(argv):
                raise ValueError(f"option {f} needs a value")
            v = argv[i + 1]; i += 2
            if f == "-k": co.min_seed_len = int(v)
            elif f == "-w": co.w = int(v)
            elif f == "-c": co.max_occ = int(v)
            elif f == "-D": co.drop_ratio = float(v)
            elif f == "-G": co.max_chain_gap = int(v)
            elif f == "-N": co.max_chain_extend = int(v)
            elif f == "-W": co.min_chain_weight = int(v)
            elif f == "-X": co.mask_level = float(v)
            elif f == "-A": co.a = ep.a = int(v)
            elif f == "-B": co.b = ep.b = int(v)
            elif f == "-O": co.o_del, co.o_ins = pair(v); ep.o_del, ep.o_ins = co.o_del, co.o_ins
            elif f == "-E": co.e_del, co.e_ins = pair(v); ep.e_del, ep.e_ins = co.e_del, co.e_ins
            elif f == "-T": po.T = int(v)
            elif f == "-h": po.max_XA_hits, po.max_XA_hits_alt = pair(v)
            elif f == "-Q": po.mapQ_coef_len = float(int(v)); po.mapQ_coef_fac = int(math.log(int(v))) if int(v) > 0 else 0
            elif f == "-U": pe.pen_unpaired = int(v)
            elif f == "-m": pe.max_matesw = int(v)
            elif f == "-R":                                             # read group (bwa_set_rg, src/bwa.c:425-452): the header line and the records' RG:Z tag
                line, rid = parse_rg_line(v, "-R")                      # (unescaped and checked by bwa_set_rg's rules)
                self.rg_line = line; self._rg_id = rid.encode(); po.rg_id = self._rg_id
                if getattr(self, "_native", None) is not None: self._native.free(); self._native = None
            elif f == "-t": self.ref_threads = int(v)                   # the reference cuts its batches at chunk_size * n_threads bases (align_file)
            elif f == "-K": self.ref_chunk_bases = int(v)               # ... or at this fixed size
            elif f in ("-l", "-v", "-f", "-d", "-L"): pass              # bookkeeping; -d -L: no effect on the GPU extension
            else:
                raise ValueError(f"option {f} is not modelled")
        if split_factor is not None: self.reseed.split_factor = float(split_factor)
        if split_width is not None: self.reseed.split_width = int(split_width)
        if max_mem_intv is not None: self.reseed.max_mem_intv = int(max_mem_intv)

    def header(self) -> str:
        """the @SQ lines and the read group's line; during a run over read groups (align_groups) every group's @RG line, in group order; during a run that keeps
        its input's read groups (align_files(keep_rg=True)) the input's @RG lines, verbatim and in file order"""
        rg = [g[0] for g in getattr(self, "_groups", None) or ()] or ([self.rg_line] if getattr(self, "rg_line", "") else [])
        return "".join(f"@SQ\tSN:{n}\tLN:{l}\n" for n, l in self.contigs) + "".join(line + "\n" for line in rg)

    def _bam_open(self, out, fmt: str, level: int, sort: bool = False) -> bool:
        """fmt="bam": checks `out` and writes the header members (bmh_bam_header of header(), compressed by the host core); True for BAM"""
        if fmt not in ("sam", "bam"):
            raise ValueError(f"fmt {fmt!r}: sam or bam")
        if fmt == "sam":
            return False
        if level not in (0, 1):
            raise ValueError(f"level {level}: 0 or 1")
        if not ("b" in getattr(out, "mode", "") or hasattr(out, "getbuffer")):
            raise ValueError('fmt="bam" needs a binary file object')
        from .lib import bam_header, bgzf_compress
        # (sorted output says so in its header: the @HD line goes in front of header()'s text, here only)
        hdr = bgzf_compress(bam_header(("@HD\tVN:1.6\tSO:coordinate\n" if sort else "") + self.header(), self.contigs), level, host=True)
        self._bam_header_bytes = len(hdr)
        out.write(hdr)
        return True

    def _bam_members(self, text: bytes, level: int) -> bytes:
        """SAM record lines -> the BGZF members of their BAM records (the device entry points); a refused record raises BamRefusal naming the read"""
        from .lib import BamRefusal, bam_status_name, bgzf_compress, sam_to_bam
        bam, st = sam_to_bam(text, self.contigs)
        bad = np.flatnonzero(st)
        if bad.size:
            line = bytes(text).split(b"\n")[int(bad[0])]
            raise BamRefusal(f"BAM output: read '{line.split(chr(9).encode())[0].decode(errors='replace')}': its SAM record cannot be written as BAM: {bam_status_name(int(st[bad[0]]))}")
        return bgzf_compress(bam, level)

    def align_batch(self, names, seqs=None, id0: int = 0, paired: bool = False, as_bytes: bool = False, quals=None, comments=None, fmt: str = "sam", level: int = 1, sort: bool = False, markdup: bool = False):
        """SAM records of one batch of reads: a ReadSet, or (names, seqs) lists of str / ASCII uint8 arrays (quals, comments: lists as
        ReadSet.from_lists takes them); id0 = index of its first read in the run.  paired: interleaved pairs (gase_aln -p); the insert-size
        statistics are the batch's.  QUAL comes from the reads' qualities, '*' without; with -C the comments end the records."""
        if markdup:
            raise ValueError("align_batch: markdup=True marks the duplicates of a sorted file, and one batch is not a file (align_file / align_files)")
        if sort:
            raise ValueError("align_batch: sort=True sorts a file's records, and one batch is not a file (align_file / align_files)")
        if fmt != "sam":                                          # fmt="bam": the batch's records as BGZF members (bytes; no header, no end-of-file member)
            if fmt != "bam" or level not in (0, 1):
                raise ValueError(f"fmt {fmt!r}, level {level}: sam or bam, 0 or 1")
            return self._bam_members(self.align_batch(names, seqs, id0=id0, paired=paired, as_bytes=True, quals=quals, comments=comments), level)
        rs = names if isinstance(names, ReadSet) else ReadSet.from_lists(names, seqs, quals=quals, comments=comments)
        self._qc = (rs.qual, rs.comments if self.po.copy_comment else None)
        L, dev, n = self.L, self.dev, len(rs)
        self._as_bytes = as_bytes
        if n == 0:
            return (np.zeros(0, np.uint8) if as_bytes == "view" else b"") if as_bytes else ""
        names = (rs.name_blob, rs.name_off)
        import time
        _t = [time.perf_counter()]; _nm = []
        def _lap(name):
            if self.profile:
                torch.cuda.synchronize(); _t.append(time.perf_counter()); _nm.append(name)
        lens, offs, ascii_ = rs.lens, np.ascontiguousarray(rs.offs), rs.ascii
        if int(lens.sum()) >= 1 << 31:
            raise ValueError("a batch holds 2^31 bases or more: offsets inside a batch are 32-bit (use a smaller batch_reads)")
        codes = rs.codes if getattr(rs, "codes", None) is not None else _NT4[ascii_]
        a_c = np.ascontiguousarray(ascii_)
        r = torch.from_numpy(a_c if a_c.flags.writeable else a_c.copy()).to(dev)        # (no copy of 150 MB per million reads unless needed)
        o = torch.from_numpy(offs.astype(np.int64)).to(torch.int32).to(dev)
        l = torch.from_numpy(lens.astype(np.int64)).to(torch.int32).to(dev)
        _lap("host prep + H2D")
        nb = max(int(lens.sum()), 1)
        ws = self._seed_ws(n, nb)
        _lap("seed workspace")
        s = ws.seed_batch(self.index, r, o, l, self.copt.min_seed_len, reseed=self.reseed if self.reseed.enable else None)
        _lap("seeding")
        e = self.ep                                             # the reference's GPU extension: deletion penalties for both gap kinds
        ext_p = ExtParams(e.a, e.b, e.o_del, e.e_del, e.o_del, e.e_del, e.zdrop, e.end_bonus)
        # the device job builder for every batch: reads beyond 700 bases are chained in wide records (chain_long_kernel), their flanks
        # extended up to the workspace's cap (768, or EXT_LONG_MAX with long_reads); HostJobs / bmh_build_jobs are the cross-check
        cw = self._chain_ws(n, max(int(s.n_seeds), 1))
        dj = cw.chain_batch(self.index, r, o, l, s)
        nr, nj = int(dj.n_regs), int(dj.n_jobs)
        out3 = torch.zeros(max(nj, 1), 3, dtype=torch.int32, device=dev)
        regs = torch.zeros(max(nr, 1), 8, dtype=torch.int32, device=dev)
        _lap("chain")
        try:
            cw.extend(out3, params=ext_p)
        except RuntimeError as err:
            _raise_beyond_cap(err)
            raise
        cw.merge(out3, regs)
        _lap("extend+merge")
        if not paired and not self.has_alt:
            # single-end: the region tail runs on the device too (bmh_finalize_regs_device); what comes back over PCIe are the records
            po = PostOpt.from_buffer_copy(self.po); po.id0 = id0
            from .lib import CapacityError, finalize_regs_device
            try:
                d_fin, d_opr = finalize_regs_device(self.index, self.copt, self.ep, po, r, o, regs, nr, dj.d_regs_per_read, dj.d_frac_rep, n,
                                                    contigs=self.contigs if len(self.contigs) > 1 else None)
            except CapacityError:
                # a read beyond the device tail's fixed limits (65 535 near-equal regions, a patch alignment of more than 1 022
                # bases): this batch takes the host form below, which has none of them -- same records
                d_fin = None
                self.host_tail_batches = getattr(self, "host_tail_batches", 0) + 1
            if d_fin is not None:
                _lap("finalize (device)")
                fin = self._d2h("fin", d_fin); opr = np.ascontiguousarray(d_opr.cpu().numpy().view(np.uint32)[:n]); m = len(fin)
                _lap("D2H records")
                self._lap = _lap; self._prof = (_t, _nm)
                return self._finish_single(names, codes, offs, lens, r, o, l, fin, opr, m, po, cw, ws, _lap, _t, _nm, as_bytes, fin_t=d_fin)
        rpr = torch.empty(n, dtype=torch.int32, device=dev); fr = torch.empty(n, dtype=torch.float32, device=dev)
        _memcpy_d2d(rpr.data_ptr(), dj.d_regs_per_read, 4 * n); _memcpy_d2d(fr.data_ptr(), dj.d_frac_rep, 4 * n)
        regs_h = np.ascontiguousarray(regs[:nr].cpu().numpy())
        rpr_h = np.ascontiguousarray(rpr.cpu().numpy().view(np.uint32)); fr_h = np.ascontiguousarray(fr.cpu().numpy())
        _lap("D2H regions")
        po = PostOpt.from_buffer_copy(self.po); po.id0 = id0
        self._lap = _lap; self._prof = (_t, _nm)
        if paired:
            return self._finish_pairs(names, codes, offs, lens, r, o, l, regs_h, rpr_h, fr_h, po, cw, ws)
        fin = np.zeros((max(nr, 1), 16), np.int32); opr = np.zeros(n, np.uint32)
        m = L.bmh_finalize_regs(C.byref(self.copt), C.byref(self.ep), C.byref(po), self.l_pac, _np_ptr(self.pac, _u8p), n, _np_ptr(codes, _u8p),
                                _np_ptr(offs, _u64p), _np_ptr(regs_h, _i32p), _np_ptr(rpr_h, _u32p), fr_h.ctypes.data_as(C.POINTER(C.c_float)),
                                len(self.contigs), self.c_off.ctypes.data_as(C.c_void_p), _np_ptr(fin, _i32p), _np_ptr(opr, _u32p), self.n_threads)
        if m < 0:
            raise RuntimeError("bmh_finalize_regs: " + (L.bmh_last_error() or b"").decode())
        fin = np.ascontiguousarray(fin[:m])
        _lap("finalize (host)")
        return self._finish_single(names, codes, offs, lens, r, o, l, fin, opr, m, po, cw, ws, _lap, _t, _nm, as_bytes)

    def _finish_single(self, names, codes, offs, lens, r, o, l, fin, opr, m, po, cw, ws, _lap, _t, _nm, as_bytes, fin_t=None):
        """records of the region tail -> CIGARs of the ones the formatter needs (device) -> SAM text (host)"""
        L, n = self.L, len(lens)
        need = np.zeros(max(m, 1), np.uint8)
        L.bmh_sam_need_cigar(C.byref(po), _np_ptr(fin, _i32p), _np_ptr(opr, _u32p), n, _np_ptr(need, _u8p))
        sel = np.nonzero(need[:m])[0].astype(np.int32)
        slot = np.full(max(m, 1), -1, np.int64); slot[sel] = np.arange(len(sel))
        aln_h, cg_h, md_h = self._cigars(r, o, l, fin, sel, fin_t=fin_t)
        _lap("cigar + D2H")
        txt = format_sam(po, names, codes, offs, lens, self.contigs, fin if m else np.zeros((1, 16), np.int32), opr, slot, aln_h, cg_h, md_h,
                         as_bytes=as_bytes, quals=self._qc[0], comments=self._qc[1])
        _lap("format (host)")
        if self.profile:
            import sys
            sys.stderr.write("[aligner] " + ", ".join("%s %.1f ms" % (nm, (_t[i + 1] - _t[i]) * 1e3) for i, nm in enumerate(_nm)) + "\n")
        return txt

    def _cigars(self, r, o, l, fin, sel, fin_t=None):
        """bmh_cigar_batch for the selected records with compact buffers; the few records that overflow them (flag 1: more
        ops, flag 8: longer MD) are redone with large ones and patched in"""
        dev = self.dev
        max_cigar, md_cap = 64, 1024
        if not len(sel):
            return np.zeros((1, 8), np.int32), np.zeros((1, max_cigar), np.uint32), np.zeros((1, md_cap), np.uint8)
        if fin_t is None or not len(fin_t):
            fin_t = torch.from_numpy(fin.copy()).to(dev)
        cg, aln, md = cigar_batch(self.index, r, o, l, fin_t, len(sel), sel_t=torch.from_numpy(sel).to(dev), params=self.ep, opt_w=self.copt.w,
                                  max_cigar=16, md_cap=96)
        aln_h = self._d2h("aln", aln)
        cg_h = self._d2h("cg", cg).view(np.uint32); md_h = self._d2h("md", md)
        over = np.flatnonzero(aln_h[:, 7] & 9)
        if over.size:
            cg_c, md_c = cg_h, md_h
            cg_h = np.zeros((len(sel), max_cigar), np.uint32); md_h = np.zeros((len(sel), md_cap), np.uint8)
            cg_h[:, :16] = cg_c; md_h[:, :96] = md_c
            cg2, aln2, md2 = cigar_batch(self.index, r, o, l, fin_t, len(over), sel_t=torch.from_numpy(sel[over].copy()).to(dev), params=self.ep,
                                         opt_w=self.copt.w, max_cigar=max_cigar, md_cap=md_cap)
            aln_h[over] = aln2.cpu().numpy(); cg_h[over] = cg2.cpu().numpy().view(np.uint32); md_h[over] = md2.cpu().numpy()
            over2 = np.flatnonzero(aln_h[:, 7] & 9)
            if over2.size and self.long_reads:
                # long regions: buffers sized from the regions themselves -- every CIGAR op takes a base of one side (at most
                # qlen + rlen ops, plus two clips), and MD holds at most a number and a base (or '^' and bases) per reference base
                rg = fin[sel[over2]]
                ql = int((rg[:, 3] - rg[:, 2]).max())
                rl = int(((rg[:, 6].astype(np.int64) & 0xFFFFFFFF | rg[:, 7].astype(np.int64) << 32)
                          - (rg[:, 4].astype(np.int64) & 0xFFFFFFFF | rg[:, 5].astype(np.int64) << 32)).max())
                mc, mdc = ql + rl + 8, 9 * rl + 16
                cg3, aln3, md3 = cigar_batch(self.index, r, o, l, fin_t, len(over2), sel_t=torch.from_numpy(sel[over2].copy()).to(dev), params=self.ep,
                                             opt_w=self.copt.w, max_cigar=mc, md_cap=mdc)
                aln3 = aln3.cpu().numpy(); cg3 = cg3.cpu().numpy().view(np.uint32); md3 = md3.cpu().numpy()
                if mc > cg_h.shape[1]:
                    cg_h = np.concatenate([cg_h, np.zeros((len(sel), mc - cg_h.shape[1]), np.uint32)], 1)
                if mdc > md_h.shape[1]:
                    md_h = np.concatenate([md_h, np.zeros((len(sel), mdc - md_h.shape[1]), np.uint8)], 1)
                aln_h[over2] = aln3; cg_h[over2] = 0; cg_h[over2, :mc] = cg3; md_h[over2] = 0; md_h[over2, :mdc] = md3
        if (aln_h[:, 7] & ~2).any():
            raise RuntimeError("bmh_cigar_batch flagged an alignment (CIGAR or MD longer than the buffers)")
        return aln_h, cg_h, md_h

    def _finish_pairs(self, names, codes, offs, lens, r, o, l, regs_h, rpr_h, fr_h, po, cw, ws) -> str:
        L, dev, n = self.L, self.dev, len(lens)
        # (the mate rescue's local alignments go to the device as one batch: bmh_finalize_pairs_dev)
        fin, opr, h_rec, unflag, _ = finalize_pairs(self.copt, self.ep, po, self.l_pac, self.pac, codes, offs, lens, regs_h, rpr_h, fr_h,
                                                    contigs=self.contigs if len(self.contigs) > 1 else None, n_threads=self.n_threads, pe=self.pe,
                                                    device=(self.index, r, o, None))
        fin = np.ascontiguousarray(fin); m = len(fin)
        need = np.zeros(max(m, 1), np.uint8)
        L.bmh_sam_need_cigar_pe(C.byref(po), _np_ptr(fin if m else np.zeros((1, 16), np.int32), _i32p), _np_ptr(np.ascontiguousarray(opr), _u32p),
                                _np_ptr(np.ascontiguousarray(h_rec), _i32p), n, _np_ptr(need, _u8p))
        sel = np.nonzero(need[:m])[0].astype(np.int32)
        slot = np.full(max(m, 1), -1, np.int64); slot[sel] = np.arange(len(sel))
        aln_h, cg_h, md_h = self._cigars(r, o, l, fin, sel)
        txt = format_sam(po, names, codes, offs, lens, self.contigs, fin if m else np.zeros((1, 16), np.int32), opr, slot, aln_h, cg_h, md_h,
                         h_rec=h_rec, unflag=unflag, as_bytes=self._as_bytes, quals=self._qc[0], comments=self._qc[1])
        return txt

    def _native_aligner(self):
        """the bmh_aligner_t of this aligner's index and options (made again when set_options changed them)"""
        from .lib import NativeAligner
        nat = getattr(self, "_native", None)
        opts = (bytes(self.copt), bytes(self.ep), bytes(self.po), bytes(self.pe))
        if nat is not None and nat.options != opts:
            nat.free(); nat = None
        if nat is None:
            nat = self._native = NativeAligner(self.index, self.pac, self.l_pac, self.contigs, self.alt if self.has_alt else None, self.copt, self.ep, self.po, self.pe)
            if self.long_reads:
                nat.set_max_qlen(EXT_LONG_MAX)
        nat.set_reseed(self.reseed if self.reseed.enable else None)
        fmt, level, sorted_keywords = self._output
        if fmt == "bam_sorted":
            if sorted_keywords.get("recal") is not None:          # the table's read groups are the run's: align_groups', keep_rg's (the input's header), else -R's, else the one group `*`
                kept = (getattr(self, "_recal_req", None) or {}).get("groups")
                groups = kept if kept else [g[1] for g in self._groups] if getattr(self, "_groups", None) else [self._rg_id.decode()] if getattr(self, "rg_line", "") else None
                sorted_keywords = dict(sorted_keywords, recal=dict(sorted_keywords["recal"], read_groups=groups))
            nat.set_sorted(level=level, **sorted_keywords)
        else:
            nat.set_output(fmt, level)
        return nat

    # what the runs that follow write: the format, the level and, for "bam_sorted", NativeAligner.set_sorted's keywords (_align_bam sets it for its run)
    _OUTPUT_DEFAULT = ("sam", 1, {})
    _output = _OUTPUT_DEFAULT

    @_coverage_keywords
    @_stats_keywords
    @_recal_keywords
    def align_file(self, reads_fa: str, out, batch_reads: int = 0, paired: bool = False, chunk_bases: int = 0, fmt: str = "sam", level: int = 1,
                   sort: bool = False, index=None, sort_mem=None, sort_tmp=None, sort_window=None, markdup: bool = False, markdup_metrics=None,
                   index_format: str = "bai", csi_min_shift: int = 14, optical_distance=None, barcode_tag=None, barcode_name=None, barcode_edits=None,
                   coverage=None, coverage_hist=None, coverage_bed=None, coverage_bin=None, coverage_min_mapq=None, coverage_deletions=False,
                    flagstat=None, idxstats=None, stats=None, insert_cap=None, recal=None, known_sites=None, recal_min_qual=None, recal_max_cycle=None, apply_recal=None, apply_recal_report=None) -> int:
        if fmt != "sam" or sort or index is not None or markdup or markdup_metrics is not None or index_format != "bai" or csi_min_shift != 14 or optical_distance is not None or barcode_tag is not None or barcode_name or barcode_edits is not None:
            return self._align_bam(lambda o: self.align_file(reads_fa, o, batch_reads=batch_reads, paired=paired, chunk_bases=chunk_bases), out, fmt, level,
                                   sort, index, sort_mem, sort_tmp, sort_window, markdup, markdup_metrics, index_format, csi_min_shift, optical_distance, barcode_tag, barcode_name, barcode_edits)
        """out: a text or binary file object.  Batches are cut the way the reference's bseq_read cuts them (src/bwa.c, called with
        chunk_size * n_threads = 10 Mbases per thread, or -K, src/fastmap.c:527): reads are added until the batch holds at least
        chunk_bases bases and an even number of reads -- in paired mode the insert-size statistics are those of the batch, so the
        cut decides flags and MAPQ of borderline pairs.  chunk_bases 0: 10 000 000 x the thread count given with -t (1).
        batch_reads > 0 cuts by read count instead (the earlier behaviour)."""
        binary = "b" in getattr(out, "mode", "") or hasattr(out, "getbuffer")
        # The file (FASTA or FASTQ) batch by batch through bmh_aligner_run_file (a loader thread cuts and fills batch k+1 .. while the lanes are on batch k:
        # nothing of the file is held beyond the batches in flight), when every read fits the device job builder (bmh_reads_scan: one counting pass);
        # BMH_ALIGNER_STREAM=0: load the whole file first (below).
        if os.environ.get("BMH_ALIGNER_NATIVE", "1") != "0" and os.environ.get("BMH_ALIGNER_STREAM", "1") != "0" and not self.profile:
            from .lib import reads_scan
            info = reads_scan(reads_fa)
            if info["n_reads"]:
                out.write(self.header().encode() if binary else self.header())
                cb = 0
                if batch_reads <= 0:
                    cb = chunk_bases or int(getattr(self, "ref_chunk_bases", 0)) or 10_000_000 * max(1, int(getattr(self, "ref_threads", 1)))
                    if not paired and not chunk_bases:
                        cb = max(cb, 150_000_000)             # (single-end records do not depend on the cuts: see below)
                    cb = min(cb, (1 << 31) - 1024)
                nat = self._native_aligner()
                try:
                    self.last_stats = nat.run_file(reads_fa, paired, (lambda mv: out.write(mv)) if binary else (lambda mv: out.write(bytes(mv).decode())),
                                                    batch_bases=cb, batch_reads=max(batch_reads, 0),
                                                    n_lanes=int(os.environ.get("BMH_ALIGNER_LANES", "3" if paired else "2")), n_threads=self.n_threads)
                except RuntimeError as e:
                    _raise_beyond_cap(e)
                    raise
                self.host_tail_batches = nat.host_tail_batches()
                return info["n_reads"]
        rs = read_reads(reads_fa, comments=bool(self.po.copy_comment))
        out.write(self.header().encode() if binary else self.header())
        n = len(rs)
        if batch_reads > 0:
            if paired:
                batch_reads -= batch_reads & 1
            cuts = list(range(0, n, batch_reads)) + [n]
        else:
            cb = chunk_bases or int(getattr(self, "ref_chunk_bases", 0)) or 10_000_000 * max(1, int(getattr(self, "ref_threads", 1)))
            if not paired and not chunk_bases:
                # single-end records do not depend on where the batches are cut (the tie-break hash takes the read's index in the run), and a
                # batch of a quarter of a million reads spends a third of its time in fixed per-batch latencies: at least 150 Mbases a batch
                cb = max(cb, 150_000_000)
            cb = min(cb, (1 << 31) - 1024)                               # offsets inside a batch are 32-bit
            csum = np.cumsum(rs.lens.astype(np.int64))
            cuts, b = [0], 0
            while b < n:
                base = csum[b - 1] if b else 0
                e = int(np.searchsorted(csum, base + cb, side="left")) + 1      # first read count whose bases reach chunk_bases
                e += (e - b) & 1                                             # ... and is even (bseq_read: size >= chunk_size && (n & 1) == 0)
                e = min(e, n)
                cuts.append(e); b = e
        # The native pipeline (csrc/align_pipeline.hip: batches driven by C threads, the text of batch k formatted while batches
        # k+1, k+2 are on the device) takes every read set whose reads fit the device job builder; BMH_ALIGNER_NATIVE=0 keeps the
        # batch-after-batch Python loop below (the same stages through the same entry points: the cross-check of the native one).
        if n and os.environ.get("BMH_ALIGNER_NATIVE", "1") != "0" and rs.codes is not None and not self.profile:
            nat = self._native_aligner()
            try:
                self.last_stats = nat.run(rs, cuts, paired, (lambda mv: out.write(mv)) if binary else (lambda mv: out.write(bytes(mv).decode())),
                                          n_lanes=int(os.environ.get("BMH_ALIGNER_LANES", "3" if paired else "2")), n_threads=self.n_threads)   # (pairs: a lane waits for host walks in the middle of its batch)
            except RuntimeError as e:
                _raise_beyond_cap(e)
                raise
            self.host_tail_batches = nat.host_tail_batches()
            return n
        for b, e in zip(cuts[:-1], cuts[1:]):
            if e > b:
                if self._output[0] == "bam_sorted":
                    raise NotImplementedError("sort=True needs the native pipeline (BMH_ALIGNER_NATIVE=0 and profile runs write batch after batch)")
                if self._output[0] == "bam":
                    out.write(self.align_batch(rs.slice(b, e), id0=b, paired=paired, fmt="bam", level=self._output[1]))
                    continue
                out.write(self.align_batch(rs.slice(b, e), id0=b, paired=paired, as_bytes="view" if binary else False))   # (binary: the library's buffer, uncopied)
        return n

    def _align_bam(self, run, out, fmt: str, level: int, sort: bool = False, index=None, sort_mem=None, sort_tmp=None, sort_window=None, markdup: bool = False, markdup_metrics=None,
                   index_format: str = "bai", csi_min_shift: int = 14, optical_distance=None, barcode_tag=None, barcode_name=None, barcode_edits=None) -> int:
        """fmt="bam" of align_file / align_files: the header members, the batches' members (`run` with the native aligner's output switched; the Python
        loop's batches converted here), the end-of-file member.  The file is written through a shim that drops the SAM header `run` writes first.
        sort=True: the batches become sorted runs and the members are those of the coordinate-sorted file, written at the end of the input; `index` (a path or
        a binary file object) receives its .bai.  markdup=True (needs sort=True): flag 0x400 on every record of every duplicate template (Picard MarkDuplicates'
        rules); self.markdup_counts holds the counts afterwards and `markdup_metrics` (a path or a text file object) receives a Picard-style table.
        index_format="csi" (needs sort=True): `index` receives a .csi in place of the .bai, with bins of 2^csi_min_shift bases (10 .. 24) -- what a
        reference with a contig of 2^29 bases or more needs; the BAM bytes do not depend on it.
        optical_distance=D (needs markdup=True; 0 .. 2^31 - 1): the decision also counts the optical duplicates -- pairs of one duplicate set that the read names
        place on one tile within D pixels in x and y.  The file and its index are byte for byte those of the run without it;
        self.markdup_optical_counts (and, over read groups, self.markdup_library_optical_counts) hold the counts, and the metrics table gains
        READ_PAIR_OPTICAL_DUPLICATES and ESTIMATED_LIBRARY_SIZE in Picard's column order.
        barcode_tag="RX" or barcode_name=True (need markdup=True; one of the two): templates with different molecular barcodes (UMIs) are no duplicates of each
        other -- the barcode is the value of that tag on the template's first record, which an aligner run carries only as the read's comment
        (so barcode_tag needs -C), or the read name's last ':' field.  self.markdup_counts gains "templates_without_barcode"; the metrics table keeps its columns.
        barcode_edits=N (needs a barcode source; 0 .. 21): barcodes within N mismatches are one molecule (packed values of at most 21 symbols of
        A C G T N - +, transitive clusters per key, the pair pass and the fragment pass each on their own).  self.markdup_counts gains "pair_barcodes_observed",
        "pair_barcodes_inferred" and "barcode_keys_skipped"; a value that does not pack fails the run by its record's index."""
        from .lib import bgzf_eof, index_format_code, optical_distance_value, barcode_source, barcode_edits_value, BARCODE_OFF, BARCODE_TAG
        barcode = barcode_source(barcode_tag, barcode_name, "align_file")
        if barcode_edits is not None and not markdup:
            raise ValueError("barcode_edits needs markdup=True: barcodes are grouped where duplicates are marked")
        edits = barcode_edits_value(barcode_edits, barcode[0], "align_file")
        if barcode[0] != BARCODE_OFF and not markdup:
            raise ValueError("barcode_tag / barcode_name need markdup=True: barcodes are compared where duplicates are marked")
        if barcode[0] == BARCODE_TAG and not self.po.copy_comment:
            raise ValueError("barcode_tag needs -C: the tag reaches a record only as the read's comment (or, from a BAM input, as its own tags under -C)")
        if optical_distance is not None:
            if not markdup:
                raise ValueError("optical_distance needs markdup=True: optical duplicates are counted where duplicates are marked")
            optical_distance = optical_distance_value(optical_distance, "align_file")
        index_format_code(index_format, csi_min_shift, "align_file")          # (csi_min_shift without "csi", a shift outside 10 .. 24: before anything is touched)
        if index_format != "bai" and not sort:
            raise ValueError(f'index_format="{index_format}" needs sort=True: only a coordinate-sorted file has an index')
        if (markdup or markdup_metrics is not None) and not sort:
            raise ValueError("markdup=True needs sort=True: duplicates are marked where the sorted file is written" if markdup else "markdup_metrics needs markdup=True and sort=True")
        if markdup_metrics is not None and not markdup:
            raise ValueError("markdup_metrics needs markdup=True")
        if sort and fmt != "bam":
            raise ValueError(f'sort=True needs fmt="bam" (fmt {fmt!r})')
        if index is not None and not sort:
            raise ValueError("index needs sort=True: only a coordinate-sorted file has a .bai")
        if fmt != "bam":
            raise ValueError(f"fmt {fmt!r}: sam or bam")
        if level not in (0, 1):
            raise ValueError(f"level {level}: 0 or 1")
        if not ("b" in getattr(out, "mode", "") or hasattr(out, "getbuffer")):
            raise ValueError('fmt="bam" needs a binary file object')
        al = self

        class _Shim:
            mode = "wb"
            first = True

            def write(self, b):
                if self.first:                                    # the SAM header text: the BAM header goes in its place
                    self.first = False
                    al._bam_open(out, "bam", level, sort)
                    return
                out.write(b)
        shim = _Shim()
        if sort:
            if os.environ.get("BMH_ALIGNER_NATIVE", "1") == "0" or self.profile:   # (before anything is switched: a refused call leaves the aligner as it was)
                raise NotImplementedError("sort=True needs the native pipeline (BMH_ALIGNER_NATIVE=0 and profile runs write batch after batch)")
        cov_req = getattr(self, "_cov_req", None) if sort else None
        stats_req = getattr(self, "_stats_req", None) if sort else None
        recal_req = getattr(self, "_recal_req", None) if sort else None
        recal_kw = None
        if recal_req is not None and recal_req["table"] is not None:      # (the mask: the known sites and the reference's holes, made once per run; the reference is the index's)
            from .lib import known_sites_mask
            mask = known_sites_mask(recal_req["known_sites"], self.contigs, l_pac=self.l_pac, holes=read_amb(self.prefix) if getattr(self, "prefix", None) else None)
            recal_kw = dict(mask=mask, min_qual=recal_req["min_qual"], max_cycle=recal_req["max_cycle"], known_sites=recal_req["known_sites"])
        if recal_req is not None and recal_req["apply"] is not None:      # the table applied to the qualities as they are written; alone, no table is counted
            recal_kw = dict(recal_kw, apply=recal_req["apply"]) if recal_kw is not None else dict(apply=recal_req["apply"], count=False)
        sorted_keywords = dict(markdup=bool(markdup), optical_distance=optical_distance, barcode_tag=barcode_tag, barcode_name=barcode_name, barcode_edits=barcode_edits,
                               index_format=index_format, csi_min_shift=int(csi_min_shift), window=int(sort_window or 0), sort_mem=sort_mem or None, sort_tmp=sort_tmp,
                               coverage=dict(min_mapq=cov_req["min_mapq"], deletions=cov_req["deletions"], bin=cov_req["bin"]) if cov_req is not None else None,
                               stats=dict(insert_cap=stats_req["insert_cap"]) if stats_req is not None else None, recal=recal_kw) if sort else {}
        self._output = ("bam_sorted" if sort else "bam", level, sorted_keywords)
        try:
            n = run(shim)
            got = self._native.sorted_results() if sort and n else {}      # (no reads: no run was made -- every part is that of a file without records)
            if cov_req is not None:
                from .lib import bam_coverage
                self.coverage = got["coverage"] if n else bam_coverage(b"", self.contigs, host=True, min_mapq=cov_req["min_mapq"], deletions=cov_req["deletions"], bin=cov_req["bin"])
            if stats_req is not None:
                from .lib import bam_stats
                self.stats = got["stats"] if n else bam_stats(b"", len(self.contigs), stats_req["insert_cap"], host=True)
            if recal_req is not None and recal_req["apply"] is not None:
                from .lib import bam_apply_recal
                self.recal_apply = got["recal"]["apply"] if n else bam_apply_recal(b"", recal_req["apply"], host=True)[1]
            if recal_req is not None and recal_req["table"] is not None:
                from .lib import bam_recal
                self.recal = got["recal"] if n else dict(bam_recal(b"", self.contigs, self.pac, self.l_pac, mask=recal_kw["mask"], min_qual=recal_req["min_qual"], max_cycle=recal_req["max_cycle"],
                                                                 host=True), known_sites=recal_req["known_sites"])
            if markdup:
                from .lib import MARKDUP_COUNTS, BARCODE_GROUP_COUNTS, OPTICAL_COUNTS
                self.markdup_counts = got["markdup_counts"] if n else dict.fromkeys(MARKDUP_COUNTS, 0)
                # per library, in order of first appearance (the library index of the run)
                libs = list(dict.fromkeys(rg_library(g[0]) for g in self._groups)) if getattr(self, "_groups", None) else []
                if libs:
                    self.markdup_library_counts = {lb: (got["markdup_library_counts"][k] if n else dict.fromkeys(MARKDUP_COUNTS, 0)) for k, lb in enumerate(libs)}
                if barcode[0] != BARCODE_OFF:
                    self.markdup_counts.update(got["markdup_barcode_counts"] if n else {"templates_without_barcode": 0})
                if edits >= 0:
                    self.markdup_counts.update(got["markdup_barcode_group_counts"] if n else dict.fromkeys(BARCODE_GROUP_COUNTS, 0))
                if optical_distance is not None:
                    self.markdup_optical_counts = got["markdup_optical_counts"] if n else dict.fromkeys(OPTICAL_COUNTS, 0)
                    self.markdup_counts.update(self.markdup_optical_counts)
                    if libs:
                        self.markdup_library_optical_counts = {lb: (got["markdup_library_optical_counts"][k] if n else dict.fromkeys(OPTICAL_COUNTS, 0)) for k, lb in enumerate(libs)}
                        for lb in libs:
                            self.markdup_library_counts[lb].update(self.markdup_library_optical_counts[lb])
        finally:
            self._output = self._OUTPUT_DEFAULT
            nat = getattr(self, "_native", None)
            if nat is not None:
                nat.set_output("sam", 1)
        if shim.first:                                            # (no reads: nothing was written)
            self._bam_open(out, "bam", level, sort)
        out.write(bgzf_eof())
        if index is not None:
            nat = self._native_aligner() if n == 0 else self._native
            if n == 0:                                            # (no run was made: the index of a file without records)
                nat.set_sorted(level=level, index_format=index_format, csi_min_shift=int(csi_min_shift)); nat.set_output("sam", 1)
            bai = nat.sort_index(self._bam_header_bytes)                 # (the bytes of the format the run was made under: .bai or .csi)
            if hasattr(index, "write"):
                index.write(bai)
            else:
                with open(index, "wb") as f:
                    f.write(bai)
        if cov_req is not None:
            if cov_req["table"] is not None:
                _write_text(cov_req["table"], coverage_table_text(self.coverage, self.contigs))
            if cov_req["hist"] is not None:
                _write_text(cov_req["hist"], coverage_hist_text(self.coverage))
            if cov_req["bed"] is not None:
                _write_text(cov_req["bed"], coverage_bed_text(self.coverage, self.contigs, cov_req["bin"]))
        if stats_req is not None:
            write_stats_texts(stats_req, self.stats, self.contigs)
        if recal_req is not None and recal_req["table"] is not None:
            from .recal import write_recal_table
            write_recal_table(self.recal, recal_req["table"])
        if recal_req is not None and recal_req["apply_report"] is not None:
            from .recal import write_recal_apply_report
            write_recal_apply_report(self.recal_apply, recal_req["apply_report"])
        if markdup_metrics is not None:
            text = markdup_metrics_text_libraries(self.markdup_library_counts) if getattr(self, "_groups", None) else markdup_metrics_text(self.markdup_counts, getattr(self, "rg_line", ""))
            if hasattr(markdup_metrics, "write"):
                markdup_metrics.write(text)
            else:
                with open(markdup_metrics, "w") as f:
                    f.write(text)
        return n

    @_coverage_keywords
    @_stats_keywords
    @_recal_keywords
    def align_files(self, reads: str, mates: str | None = None, out=None, paired: bool = False, chunk_bases: int = 0, batch_reads: int = 0, fmt: str = "sam", level: int = 1,
                    sort: bool = False, index=None, sort_mem=None, sort_tmp=None, sort_window=None, markdup: bool = False, markdup_metrics=None, keep_rg: bool = False,
                    index_format: str = "bai", csi_min_shift: int = 14, optical_distance=None, barcode_tag=None, barcode_name=None, barcode_edits=None,
                    collate: bool = False, collate_mem=None,
                    coverage=None, coverage_hist=None, coverage_bed=None, coverage_bin=None, coverage_min_mapq=None, coverage_deletions=False,
                    flagstat=None, idxstats=None, stats=None, insert_cap=None, recal=None, known_sites=None, recal_min_qual=None, recal_max_cycle=None, apply_recal=None, apply_recal_report=None) -> int:
        """apply_recal= (a path to a table recal= wrote, or read_recal_table's dict; needs sort=True): the base qualities of every record are recalibrated by that
        table as the sorted file is written, on the device in every window of the final merge behind its flag step; coverage, the statistics and
        recal= then see the qualities as written (recal= gives the "after" table; it may not name the same file), while markdup's choice rests on the original
        qualities.  apply_recal_report= (a path or a text file object): recal_apply_report_text's rows.  self.recal_apply holds the counts afterwards.
        recal= (a path or a text file object; needs sort=True): the covariate table of base quality score recalibration of the file being written (DESIGN.md
        4.16; recal_table_text's rows), counted on the device from every window of the final merge behind its flag step against the index's own reference, under
        known_sites= (VCF or BED files, plain or gzip; the reference's holes are always masked), recal_min_qual= (6) and recal_max_cycle= (500).  The read groups
        are the run's (-R, align_groups'; with keep_rg=True the @RG lines of the input's header, which is read ahead of the run: a file, not a pipe).  self.recal holds the arrays afterwards (bam_recal's dict).
        flagstat=, idxstats=, stats= (paths or text file objects; need sort=True): `samtools flagstat`'s and `samtools idxstats`' texts and a sectioned summary with
        mapq and insert-size histograms (stats_text) of the file being written, computed on the device from every window of the final merge behind its flag step
        (DESIGN.md 4.15), so with the 0x400 flags markdup=True sets; insert_cap=N (2 .. 65536): sizes from N up share the last bin.  self.stats holds the arrays
        afterwards (bam_stats' dict).  The BAM and its index are byte for byte those of the run without them.
        coverage=, coverage_hist=, coverage_bed= (paths or text file objects; need sort=True): the coverage depth of the file being written, computed on the
        device from every window of the final merge behind its flag step -- duplicates that markdup=True marks are counted out.  They receive
        coverage_table_text, coverage_hist_text and coverage_bed_text (the last with coverage_bin=N positions a row); coverage_min_mapq=Q and coverage_deletions=True
        say what counts.  self.coverage holds the arrays afterwards (bam_coverage's dict).  The BAM and its index are byte for byte those of the run without them.
        align_file for the files users have (bmh_aligner_run_files): `reads` (and `mates`: the second file of a pair, which implies paired) may be
        multi-line FASTA or FASTQ, plain, gzip or BGZF, a regular file or a pipe; or `reads` alone is a BAM file (unaligned, or grouped by read name: recognised
        from its bytes, pairs from flag 0x1 of its records -- paired=True on a BAM without it is refused).  Batches are cut by align_file's rules (-t, -K, the 150 Mbase floor for
        single-end runs), so the text equals align_file's on the single-line interleaved file of the same reads.  Returns the number of reads.
        keep_rg=True keeps the input's read groups: `reads` is one BAM (a regular file or a pipe), the @RG lines of its header are the run's read groups and go
        verbatim, in file order, where -R's line goes in the output header, and every read's records carry RG:Z:<the ID its own record names> where -R's tag goes.
        Batches are cut and reads indexed as without it, and a batch may hold reads of any number of groups.  markdup=True calls duplicates within a library (the
        LB field, rg_library's rules): self.markdup_library_counts and markdup_metrics have a row per library.  Refused before anything is written (ValueError):
        text input, `mates`, -R, a header without a valid @RG line (bam_read_groups' rules).  A record without an RG:Z tag, with an ID the header does not hold,
        or a pair of two groups fails the run naming the record's index, after the batches before it were written.
        collate=True takes a paired BAM in any record order, a coordinate-sorted one -- this aligner's own sort=True output -- among them: the mates of a pair are
        found by name on the device (bmh_aligner_set_collate; include/bwamem_hip.h has the definition), the reads are the pairs in the order in which their later
        record comes, and the output is byte for byte that of a run without it on the name-grouped BAM of the same pairs in that order.  It composes with every
        other option and changes none.  collate_mem: the cap in bytes on the records that wait for their partners (None: 8 GiB; needs collate); beyond it, and at
        a record whose partner never comes, the run fails naming the record after the batches before it were written.  Text input is refused before anything is
        written (a regular file is looked at first; a pipe of text is refused by the library once it is opened)."""
        if out is None:
            raise ValueError("align_files: out (a text or binary file object) is required")
        if collate_mem is not None and not collate:
            raise ValueError("align_files: collate_mem without collate=True: the cap is that of the collation's open records")
        if collate and getattr(self, "_collate", None) is None:        # the outermost call of such a run: the refusals, and the state that lasts as long as it
            if mates is not None or _holds_bam(reads) is False:
                from .lib import ReadFileError
                raise ReadFileError(f"reads file: {reads}: mates are collated by name (--collate) in BAM input only: text input is taken in the order of its records")
            if os.environ.get("BMH_ALIGNER_NATIVE", "1") == "0" or self.profile:
                raise NotImplementedError("collate=True needs the native pipeline (BMH_ALIGNER_NATIVE=0 and profile runs write batch after batch)")
            self._collate = (True, collate_mem)
            try:
                return self.align_files(reads, None, out=out, paired=paired, chunk_bases=chunk_bases, batch_reads=batch_reads, fmt=fmt, level=level, sort=sort, index=index,
                                        sort_mem=sort_mem, sort_tmp=sort_tmp, sort_window=sort_window, markdup=markdup, markdup_metrics=markdup_metrics, keep_rg=keep_rg,
                                        index_format=index_format, csi_min_shift=csi_min_shift, optical_distance=optical_distance, barcode_tag=barcode_tag, barcode_name=barcode_name, barcode_edits=barcode_edits)
            finally:
                self._collate = None
                nat = getattr(self, "_native", None)
                if nat is not None:
                    nat.set_collate(False)
        if keep_rg and getattr(self, "_keep_rg", None) is None:          # the outermost call of such a run: the refusals, and the state that lasts as long as it
            if mates is not None:
                raise ValueError("align_files: keep_rg=True and a mates file: a run that keeps its input's read groups takes one BAM file")
            if getattr(self, "rg_line", ""):
                raise ValueError("align_files: keep_rg=True and -R is set: the read groups come from the input's header or from -R, not both")
            if os.environ.get("BMH_ALIGNER_NATIVE", "1") == "0" or self.profile:
                raise NotImplementedError("keep_rg=True needs the native pipeline (BMH_ALIGNER_NATIVE=0 and profile runs write batch after batch)")
            self._keep_rg = True
            try:
                return self.align_files(reads, None, out=out, paired=paired, chunk_bases=chunk_bases, batch_reads=batch_reads, fmt=fmt, level=level, sort=sort, index=index,
                                        sort_mem=sort_mem, sort_tmp=sort_tmp, sort_window=sort_window, markdup=markdup, markdup_metrics=markdup_metrics, keep_rg=True,
                                        index_format=index_format, csi_min_shift=csi_min_shift, optical_distance=optical_distance, barcode_tag=barcode_tag, barcode_name=barcode_name, barcode_edits=barcode_edits)
            finally:
                self._keep_rg = None
                self._groups = None
                nat = getattr(self, "_native", None)
                if nat is not None:
                    nat.set_keep_rg(False)
        if fmt != "sam" or sort or index is not None or markdup or markdup_metrics is not None or index_format != "bai" or csi_min_shift != 14 or optical_distance is not None or barcode_tag is not None or barcode_name or barcode_edits is not None:
            return self._align_bam(lambda o: self.align_files(reads, mates, out=o, paired=paired, chunk_bases=chunk_bases, batch_reads=batch_reads, keep_rg=keep_rg), out, fmt, level,
                                   sort, index, sort_mem, sort_tmp, sort_window, markdup, markdup_metrics, index_format, csi_min_shift, optical_distance, barcode_tag, barcode_name, barcode_edits)
        binary = "b" in getattr(out, "mode", "") or hasattr(out, "getbuffer")
        paired = bool(paired or mates is not None)
        cb = 0
        if batch_reads <= 0:
            cb = chunk_bases or int(getattr(self, "ref_chunk_bases", 0)) or 10_000_000 * max(1, int(getattr(self, "ref_threads", 1)))
            if not paired and not chunk_bases:
                cb = max(cb, 150_000_000)                 # (single-end records do not depend on the cuts: align_file)
            cb = min(cb, (1 << 31) - 1024)
        nat = self._native_aligner()
        nat.set_collate(*(getattr(self, "_collate", None) or (False, None)))
        if keep_rg:
            # the header waits for the input's: the library calls back once it has read the BAM's header whole -- before the first record -- and the @RG lines go
            # into ours there (header() reads self._groups); a refused input has written nothing by then
            def rg_header(lines, _libs):
                self._groups = [(ln, next(f[3:] for f in ln.split("\t")[1:] if f.startswith("ID:")), None, None) for ln in lines]
                out.write(self.header().encode() if binary else self.header())
            nat.set_keep_rg(True, rg_header)
        else:
            out.write(self.header().encode() if binary else self.header())
        # (a BAM says itself whether it holds pairs, once the library has opened it: the batch size and lanes of a paired run, for that case)
        cb_pairs = 0 if batch_reads > 0 else min(chunk_bases or int(getattr(self, "ref_chunk_bases", 0)) or 10_000_000 * max(1, int(getattr(self, "ref_threads", 1))), (1 << 31) - 1024)
        nat.set_bam_pairs(cb_pairs, int(os.environ.get("BMH_ALIGNER_LANES", "3")))
        try:
            self.last_stats = nat.run_files(reads, mates, paired, (lambda mv: out.write(mv)) if binary else (lambda mv: out.write(bytes(mv).decode())),
                                             batch_bases=cb, batch_reads=max(batch_reads, 0),
                                             n_lanes=int(os.environ.get("BMH_ALIGNER_LANES", "3" if paired else "2")), n_threads=self.n_threads)
        except RuntimeError as e:
            _raise_beyond_cap(e)
            raise
        self.host_tail_batches = nat.host_tail_batches()
        return int(self.last_stats.n_reads)

    @_coverage_keywords
    @_stats_keywords
    @_recal_keywords
    def align_groups(self, groups, out=None, paired: bool = False, chunk_bases: int = 0, batch_reads: int = 0, fmt: str = "sam", level: int = 1,
                     sort: bool = False, index=None, sort_mem=None, sort_tmp=None, sort_window=None, markdup: bool = False, markdup_metrics=None,
                     index_format: str = "bai", csi_min_shift: int = 14, optical_distance=None, barcode_tag=None, barcode_name=None, barcode_edits=None,
                     collate: bool = False, collate_mem=None,
                     coverage=None, coverage_hist=None, coverage_bed=None, coverage_bin=None, coverage_min_mapq=None, coverage_deletions=False,
                    flagstat=None, idxstats=None, stats=None, insert_cap=None, recal=None, known_sites=None, recal_min_qual=None, recal_max_cycle=None, apply_recal=None, apply_recal_report=None) -> int:
        """several read groups -- a sample's lanes and libraries -- into one output (bmh_aligner_run_groups).  groups: [(rg_line, reads, mates or None), ...]; every
        rg_line is unescaped and checked as -R's value is, reads / mates are what align_files takes (one file or R1 + R2; plain, gzip or BGZF; FASTA or FASTQ; or
        one BAM, whose own @RG lines and RG tags stay ignored: align_files(keep_rg=True) is the run that keeps them, and the two do not combine).  Group g's records are byte for byte those of align_files(reads_g, mates_g) alone under -R rg_g, and
        the unsorted output is the groups' outputs in order; the header holds every @RG line.  All groups hold pairs or none does (paired applies to every group).
        markdup=True calls duplicates within a library only (a group's library is its LB field; groups without one share "Unknown Library"):
        self.markdup_library_counts holds the counts per library, markdup_metrics one row per library.  Needs the native pipeline; -R must not be set.
        collate / collate_mem: align_files' -- they apply to every group whose input is one BAM; groups of text files are taken as ever.
        coverage / coverage_hist / coverage_bed / coverage_bin / coverage_min_mapq / coverage_deletions: align_files' -- the coverage is the whole file's, not per library.
        flagstat / idxstats / stats / insert_cap: align_files' -- the statistics are the whole file's, not per read group or library.
        Returns the number of reads."""
        if out is None:
            raise ValueError("align_groups: out (a text or binary file object) is required")
        if collate_mem is not None and not collate:
            raise ValueError("align_groups: collate_mem without collate=True: the cap is that of the collation's open records")
        if not groups:
            raise ValueError("align_groups: no read groups were given")
        if getattr(self, "rg_line", ""):
            raise ValueError("align_groups: -R is set: a run over read groups takes its read groups from `groups` alone")
        parsed = []
        for k, g in enumerate(groups):
            if len(g) not in (2, 3) or g[1] is None:
                raise ValueError(f"align_groups: group {k}: (rg_line, reads, mates or None)")
            line, rid = parse_rg_line(g[0], f"align_groups: group {k}")
            if any(rid == q[1] for q in parsed):
                raise ValueError(f"align_groups: group {k}: the read group ID '{rid}' is given twice")
            parsed.append((line, rid, g[1], g[2] if len(g) == 3 else None))
        libs = list(dict.fromkeys(rg_library(q[0]) for q in parsed))
        if len(libs) > 255:
            raise ValueError(f"align_groups: {len(libs)} libraries: a run holds at most 255 (the library is a byte of the duplicate key)")
        if os.environ.get("BMH_ALIGNER_NATIVE", "1") == "0" or self.profile:
            raise NotImplementedError("align_groups needs the native pipeline (BMH_ALIGNER_NATIVE=0 and profile runs write batch after batch)")
        self._groups = parsed
        self._collate = (True, collate_mem) if collate else None
        try:
            if fmt != "sam" or sort or index is not None or markdup or markdup_metrics is not None or index_format != "bai" or csi_min_shift != 14 or optical_distance is not None or barcode_tag is not None or barcode_name or barcode_edits is not None:
                return self._align_bam(lambda o: self._run_groups(parsed, libs, o, paired, chunk_bases, batch_reads), out, fmt, level,
                                       sort, index, sort_mem, sort_tmp, sort_window, markdup, markdup_metrics, index_format, csi_min_shift, optical_distance, barcode_tag, barcode_name, barcode_edits)
            return self._run_groups(parsed, libs, out, paired, chunk_bases, batch_reads)
        finally:
            self._groups = None
            self._collate = None
            nat = getattr(self, "_native", None)
            if nat is not None:
                nat.set_collate(False)

    def _run_groups(self, parsed, libs, out, paired, chunk_bases, batch_reads) -> int:
        binary = "b" in getattr(out, "mode", "") or hasattr(out, "getbuffer")
        stated = bool(paired or any(q[3] is not None for q in parsed))             # (pairs by what the caller says; a BAM says the rest itself: align_files)
        cb_pairs = 0 if batch_reads > 0 else min(chunk_bases or int(getattr(self, "ref_chunk_bases", 0)) or 10_000_000 * max(1, int(getattr(self, "ref_threads", 1))), (1 << 31) - 1024)
        cb = cb_pairs
        if batch_reads <= 0 and not stated and not chunk_bases:
            cb = min(max(cb, 150_000_000), (1 << 31) - 1024)                       # (single-end records do not depend on the cuts: align_file)
        for _line, rid, reads, mates in parsed:                                    # (before the header is written: a refused run leaves `out` empty)
            for path in (reads, mates):
                if path is not None and not os.path.exists(path):
                    from .lib import ReadFileError
                    raise ReadFileError(f"read group '{rid}': reads file: {path}: no such file")
        out.write(self.header().encode() if binary else self.header())
        nat = self._native_aligner()
        nat.set_collate(*(getattr(self, "_collate", None) or (False, None)))
        nat.set_bam_pairs(cb_pairs, int(os.environ.get("BMH_ALIGNER_LANES", "3")))
        try:
            self.last_stats = nat.run_groups([(q[1], libs.index(rg_library(q[0])), q[2], q[3]) for q in parsed], bool(paired),
                                             (lambda mv: out.write(mv)) if binary else (lambda mv: out.write(bytes(mv).decode())), batch_bases=cb, batch_reads=max(batch_reads, 0),
                                             n_lanes=int(os.environ.get("BMH_ALIGNER_LANES", "3" if stated else "2")), n_threads=self.n_threads)
        except RuntimeError as e:
            _raise_beyond_cap(e)
            raise
        self.host_tail_batches = nat.host_tail_batches()
        return int(self.last_stats.n_reads)

    # The seeding and chaining workspaces are kept between batches (allocating and freeing a few GB of HBM per batch cost more than
    # the kernels of an easy batch); a batch that needs more gets a new one, a quarter larger than it asked for.
    def _d2h(self, key: str, t):
        """device tensor -> numpy array in a PINNED host buffer kept per key (one DMA instead of a staged pageable copy: the CIGAR /
        MD / record arrays of a million reads are 200 MB).  The array is valid until the next call with the same key."""
        t = t.contiguous()
        nbytes = t.numel() * t.element_size()
        if nbytes == 0:
            return t.cpu().numpy()
        c = getattr(self, "_pin", None)
        if c is None:
            c = self._pin = {}
        buf = c.get(key)
        if buf is None or buf.numel() < nbytes:
            buf = c[key] = torch.empty(nbytes + nbytes // 4, dtype=torch.uint8, pin_memory=True)
        dst = buf[:nbytes].view(t.dtype).view(t.shape)
        dst.copy_(t, non_blocking=True)
        torch.cuda.current_stream(t.device).synchronize()
        return dst.numpy()

    def _seed_ws(self, n: int, nb: int):
        c = getattr(self, "_ws_cache", None)
        if c is not None and n <= c[1] and nb <= c[2]:
            return c[0]
        if c is not None:
            c[0].free()
        cn, cb = (n, nb) if c is None else (n + n // 4, nb + nb // 4)
        ws = SeedWorkspace(cn, cb, max_cands=cb, max_occ=max(64 * cn, 1 << 16))       # one candidate per base bounds the candidates; the workspace adds what its chunked appends lose
        self._ws_cache = (ws, cn, cb)
        return ws

    def _chain_ws(self, n: int, n_seeds: int):
        c = getattr(self, "_cw_cache", None)
        if c is not None and n <= c[1] and n_seeds <= c[2]:
            return c[0]
        if c is not None:
            c[0].free()
        cn, cs = (n, n_seeds + n_seeds // 8) if c is None else (n + n // 4, n_seeds + n_seeds // 4)
        cw = ChainWorkspace(cn, cs, opt=self.copt)
        cw.set_materialize(False)
        if self.long_reads:
            cw.set_max_qlen(EXT_LONG_MAX)
        if len(self.contigs) > 1:
            cw.set_contigs(self.contigs)
            if self.has_alt:
                cw.set_alt(self.alt)
        self._cw_cache = (cw, cn, cs)
        return cw

    def __del__(self):                      # an Aligner dropped without close() must not keep its workspaces in HBM
        try:
            for nm in ("_ws_cache", "_cw_cache"):
                c = getattr(self, nm, None)
                if c is not None:
                    c[0].free(); setattr(self, nm, None)
        except Exception:
            pass

    def close(self):
        nat = getattr(self, "_native", None)
        if nat is not None:
            nat.free(); self._native = None
        for nm in ("_ws_cache", "_cw_cache"):
            c = getattr(self, nm, None)
            if c is not None:
                c[0].free(); setattr(self, nm, None)
        self.index.free()
