"""`bwa mem` on the device: reads (FASTA or FASTQ, multi-line or not, plain, gzip or BGZF, one file or an R1 / R2 pair; or one BAM file, unaligned or
grouped by read name, which says itself whether it holds pairs) -> SAM.

    python -m bwamem_hip.mem [options] PREFIX reads [mates] [-o out.sam]
    python -m bwamem_hip.mem [options] PREFIX --rg LINE reads [mates] --rg LINE reads [mates] ... [-o out.sam]

PREFIX is what `python -m bwamem_hip.index` (or `bwa index`) wrote.  Options are Aligner.set_options' list (-k -w -c -D -G -N -W -X -A -B
-O -E -T -h -Q -U -m -R -a -M -Y -S -P -j -C -g -t -K ...) plus -p (the one file holds interleaved pairs), -o (the output file; default
stdout), --long-reads (reads of up to 16 384 bases), --device (the torch device, cuda:0), --bam (the output is BAM: records converted and BGZF-
compressed on the device; -o is unchanged, a name ending in .bam does not switch formats), --bam-level 0|1 (stored, or LZ77 + dynamic Huffman; 1),
--sort (implies --bam: the records in coordinate order, `samtools sort`'s, sorted on the device; with -o PATH the BAI index goes to PATH.bai, --index PATH
names it otherwise, and on stdout without --index none is written), --sort-mem BYTES (records kept in host memory before the sorted runs spill to a temporary
file; 4 GiB), --sort-tmp DIR (where that file lives; $TMPDIR, else /tmp), --csi (implies --sort: the index is a CSI index, which a reference with a contig
of 2^29 bases or more needs -- a BAI cannot hold one, and --sort alone refuses it; with -o PATH it goes to PATH.csi, --index PATH names it otherwise; the BAM
bytes are those of --sort), --csi-min-shift N (needs --csi: the index's smallest bins and windows hold 2^N bases, 10 .. 24; 14, as in a BAI), --markdup
(needs --sort: flag 0x400 on every record of every duplicate template,
decided on the device by Picard MarkDuplicates' rules -- the unclipped 5' ends and strands of a template's primary lines are the key, the sum of the base
qualities >= 15 the score, ties go to the template that came first in the input, a fragment is a duplicate wherever a pair has an end; unlike Picard and
`samtools markdup` on coordinate-sorted input the secondary and supplementary lines of a duplicate template are flagged too; nothing is removed, no DT:Z
tag is written; with --csi a contig beyond 2^30 - 2^24 bases is refused for --markdup, by name), --markdup-metrics PATH
(a Picard-style table of the counts, one row per library) and --optical-distance N (needs --markdup; a whole number, 0 .. 2^31 - 1 -- Picard uses 100, and 2500
on patterned flow cells; there is no default: the option turns the step on -- the decision also counts the optical duplicates: pairs of one duplicate set whose
read names, Illumina's 5 or 7 ':'-separated fields ending in tile:x:y, place them on one tile of one read group within N pixels in x and in y, clusters being
the connected components; the BAM and its index stay byte for byte those of --markdup, and the metrics table gains READ_PAIR_OPTICAL_DUPLICATES and
ESTIMATED_LIBRARY_SIZE in Picard's column order; the names' pattern is fixed), --barcode-tag XX and --barcode-name (need --markdup; one of the two: templates
with different molecular barcodes -- UMIs -- are no duplicates of each other, as with Picard's BARCODE_TAG and `samtools markdup --barcode-tag / --barcode-name`.
--barcode-tag XX: the barcode is the value of tag XX, type Z, on a template's first record, taken verbatim (a dual UMI ACGT-TTGA is one value); it needs -C,
which copies a FASTQ comment such as RX:Z:ACGT, or a uBAM's own tags, into the records; XX is two characters [A-Za-z][A-Za-z0-9], not RG nor a tag the aligner
writes itself.  --barcode-name: the barcode is what follows the last ':' of the read name, bcl-convert's ...:tile:x:y:UMI, and --optical-distance then locates a
read by the name without that field.  A template without a barcode is comparable only with others without one; barcodes are compared exactly unless
--barcode-edits N is given; the metrics table keeps its columns), --barcode-edits N (needs --barcode-tag or --barcode-name; a whole number, 0 .. 21 -- Picard's
UmiAwareMarkDuplicatesWithMateCigar uses 1: barcodes within N mismatches are one molecule.  The barcodes at one pair of ends are clustered transitively and
compared by their cluster's smallest; those at one end likewise, on their own, before the fragment rule.  A barcode holds at most 21 bytes of A C G T N - +:
any other value, lower case included, fails the run by its record's index; barcodes of different lengths are never joined, and a key with more than 65 536
distinct barcodes is left exact; no MI or DT tag is written).  --rg LINE opens a read group:
LINE is an @RG line as -R takes it, and the one or two files that follow it, up to the next --rg, are that group's input (Aligner.align_groups): a sample's lanes
and libraries go into one output, every record with its group's RG:Z, the header with every @RG line, and --markdup calls duplicates within a library (the LB
field; groups with one LB are lanes of one library) only.  -p applies to every group; --rg and -R exclude each other.  --keep-rg keeps the read groups of the
input, one BAM file (Aligner.align_files(keep_rg=True)): the @RG lines of its header go into the output's header verbatim, every read's records carry the RG:Z of
the read's own record, and --markdup calls duplicates within a library; it is refused on text input, with a mates file, and beside -R or --rg.  --collate takes a
paired BAM in any record order -- a coordinate-sorted one, this program's own --sort output among them: the mates of a pair are found by name on the device, the
reads are the pairs in the order in which their later record comes, and the output is byte for byte that of a run on the name-grouped BAM of the same pairs in
that order (Aligner.align_files(collate=True)); first mates wait for their partners in host memory, at most --collate-mem BYTES of them (needs --collate; 8 GiB by
default; nothing is spilled to disk: beyond the cap the run stops after the batches before it, naming the record); a record whose partner never comes is refused
after the complete batches; text input is refused (a regular file before anything is written, a pipe of text after the header); with --rg it applies to every group whose input is a BAM.
--coverage PATH, --coverage-hist PATH and --coverage-bed PATH (need --sort) write the coverage depth of the file being written, computed on the device while it
is written: `samtools coverage`'s table (one row per contig and a row `total`), the depth histogram (depth, bases, fraction at or above; the last row 1000+) and
the mean depth of every --coverage-bin N positions (--coverage-bed and --coverage-bin go together).  A record counts by `samtools depth`'s default filters --
unmapped, secondary, QC-failed and duplicate records are out, so --markdup's duplicates are counted out; supplementary records count -- and with
--coverage-min-mapq Q (0 .. 255) only at mapq >= Q; it covers the positions under M, = and X, and under D with --coverage-deletions (`samtools depth -J`).
There is no base-quality filter and no correction for overlapping mates.  With --rg the coverage is the whole file's, not per library.
--flagstat PATH, --idxstats PATH and --stats PATH (need --sort) write `samtools flagstat`'s sixteen lines, `samtools idxstats`' table and a sectioned summary (flag
and contig counts, reads, bases, operations, NM, the mapq histogram, the insert-size histogram per orientation and its median, MAD, mode, mean and SD) of the
file being written, computed on the device while it is written, from the records in their final order with --markdup's final 0x400 flags.  The statistics are
the whole file's, not per read group or library.
--recal PATH (needs --sort) writes the covariate table of base quality score recalibration -- observations and errors by read group, quality, cycle and context,
for mismatches, insertions and deletions (GATK BaseRecalibrator's counting rules at its default covariates, restated; BAQ off, no adaptor clipping)
-- counted on the device while the file is written, against the index's own reference, with --markdup's duplicates counted out.  --known-sites FILE (repeatable;
VCF or BED, plain or gzip) masks known variants, the reference's holes (.amb) are always masked; --recal-min-qual Q (0 .. 93; 6) and --recal-max-cycle N
(1 .. 65535; 500).  --apply-recal TABLE (needs --sort) recalibrates the base qualities of every record by a table --recal wrote, on the device while the file
is written (GATK ApplyBQSR's hierarchical model over mismatches, restated; no OQ tag, no quantisation); --recal in the same run then counts the
"after" table of the qualities as written (another file than TABLE), and --markdup's choice rests on the original qualities.  --apply-recal-report PATH writes
what changed (rows `AS name value`, `AQ quality before after`).  The read groups are -R's, --rg's or, with --keep-rg, the @RG lines of the input's header (read ahead of the run: a file, not a pipe).  An option that is
not on that list is refused by name.  Two input files imply pairs.  One plain, regular file is offered to Aligner.align_file first, which takes it when every
record has one sequence line (its own counting pass decides, before anything is written); every other input goes through
Aligner.align_files; the text is the same.  A refused file ends the command with status 1 and the library's message on stderr.
"""
from __future__ import annotations

import os
import stat
import sys

FLAGS = ("-a", "-M", "-Y", "-S", "-P", "-j", "-C", "-g")
VALUED = ("-k", "-w", "-c", "-D", "-G", "-N", "-W", "-X", "-A", "-B", "-O", "-E", "-T", "-h", "-Q", "-U", "-m", "-R", "-t", "-K", "-l", "-v", "-f", "-d", "-L")


def _plain_regular(path: str) -> bool:
    """a regular, uncompressed file: what align_file's mapped loader can take (whether its records are single-line is align_file's to say)"""
    try:
        if not stat.S_ISREG(os.stat(path).st_mode):
            return False
        with open(path, "rb") as f:
            return f.read(2) != b"\x1f\x8b"
    except OSError:
        return False


def main(argv=None) -> int:
    argv = list(sys.argv[1:] if argv is None else argv)
    opts, pos, out_path, interleaved, long_reads, device = [], [], None, False, False, "cuda:0"
    bam, bam_level = False, 1
    sort, index_path, sort_mem, sort_tmp = False, None, None, None
    markdup, metrics_path, optical = False, None, None
    barcode_tag, barcode_name, barcode_edits = None, False, None
    csi, csi_shift = False, None
    keep_rg = False
    collate, collate_mem = False, None
    cov_paths, cov_bin, cov_mapq, cov_del = {}, None, None, False
    stats_paths = {}
    recal_kw, recal_sites, apply_kw = {}, [], {}
    groups = []                                                     # --rg LINE: [line, files...]; the positionals behind it are its files
    i = 0
    while i < len(argv):
        a = argv[i]
        if a == "-p":
            interleaved = True
        elif a == "--long-reads":
            long_reads = True
        elif a == "--bam":
            bam = True
        elif a == "--bam-level":
            if i + 1 >= len(argv) or argv[i + 1] not in ("0", "1"):
                print("[bwamem_hip.mem] option --bam-level needs 0 or 1", file=sys.stderr)
                return 2
            bam_level = int(argv[i + 1])
            i += 1
        elif a == "--sort":
            sort = bam = True
        elif a == "--markdup":
            markdup = True
        elif a == "--csi":
            csi = sort = bam = True
        elif a == "--csi-min-shift":
            if i + 1 >= len(argv) or not argv[i + 1].isdigit() or not 10 <= int(argv[i + 1]) <= 24:
                print("[bwamem_hip.mem] option --csi-min-shift needs a number in 10 .. 24", file=sys.stderr)
                return 2
            csi_shift = int(argv[i + 1])
            i += 1
        elif a == "--optical-distance":
            if i + 1 >= len(argv) or not (argv[i + 1].isascii() and argv[i + 1].isdigit()) or int(argv[i + 1]) > 0x7fffffff:
                print("[bwamem_hip.mem] option --optical-distance needs a whole number of pixels, 0 .. 2^31 - 1", file=sys.stderr)
                return 2
            optical = int(argv[i + 1])
            i += 1
        elif a == "--barcode-edits":
            if i + 1 >= len(argv) or not (argv[i + 1].isascii() and argv[i + 1].isdigit()) or int(argv[i + 1]) > 21:
                print("[bwamem_hip.mem] option --barcode-edits needs a whole number of mismatches, 0 .. 21", file=sys.stderr)
                return 2
            barcode_edits = int(argv[i + 1])
            i += 1
        elif a == "--barcode-name":
            barcode_name = True
        elif a == "--barcode-tag":
            if i + 1 >= len(argv):
                print("[bwamem_hip.mem] option --barcode-tag needs a tag of two characters", file=sys.stderr)
                return 2
            barcode_tag = argv[i + 1]
            i += 1
        elif a == "--keep-rg":
            keep_rg = True
        elif a == "--collate":
            collate = True
        elif a == "--collate-mem":
            if i + 1 >= len(argv) or not (argv[i + 1].isascii() and argv[i + 1].isdigit()) or int(argv[i + 1]) < 1:
                print("[bwamem_hip.mem] option --collate-mem needs a number of bytes", file=sys.stderr)
                return 2
            collate_mem = int(argv[i + 1])
            i += 1
        elif a in ("--coverage", "--coverage-hist", "--coverage-bed"):
            if i + 1 >= len(argv):
                print(f"[bwamem_hip.mem] option {a} needs a value", file=sys.stderr)
                return 2
            cov_paths[a] = argv[i + 1]
            i += 1
        elif a in ("--recal", "--known-sites", "--recal-min-qual", "--recal-max-cycle"):
            if i + 1 >= len(argv):
                print(f"[bwamem_hip.mem] option {a} needs a value", file=sys.stderr)
                return 2
            if a == "--known-sites":
                recal_sites.append(argv[i + 1])
            elif a == "--recal":
                recal_kw["recal"] = argv[i + 1]
            else:
                lo, hi = (0, 93) if a == "--recal-min-qual" else (1, 65535)
                if not (argv[i + 1].isascii() and argv[i + 1].isdigit()) or not lo <= int(argv[i + 1]) <= hi:
                    print(f"[bwamem_hip.mem] option {a} needs a whole number, {lo} .. {hi}", file=sys.stderr)
                    return 2
                recal_kw[a[2:].replace("-", "_")] = int(argv[i + 1])
            i += 1
        elif a in ("--apply-recal", "--apply-recal-report"):
            if i + 1 >= len(argv):
                print(f"[bwamem_hip.mem] option {a} needs a value", file=sys.stderr)
                return 2
            apply_kw[a[2:].replace("-", "_")] = argv[i + 1]
            i += 1
        elif a in ("--flagstat", "--idxstats", "--stats"):
            if i + 1 >= len(argv):
                print(f"[bwamem_hip.mem] option {a} needs a value", file=sys.stderr)
                return 2
            stats_paths[a] = argv[i + 1]
            i += 1
        elif a == "--coverage-bin":
            if i + 1 >= len(argv) or not (argv[i + 1].isascii() and argv[i + 1].isdigit()) or not 1 <= int(argv[i + 1]) <= 0xffffffff:
                print("[bwamem_hip.mem] option --coverage-bin needs a whole number of positions, 1 .. 2^32 - 1", file=sys.stderr)
                return 2
            cov_bin = int(argv[i + 1])
            i += 1
        elif a == "--coverage-min-mapq":
            if i + 1 >= len(argv) or not (argv[i + 1].isascii() and argv[i + 1].isdigit()) or int(argv[i + 1]) > 255:
                print("[bwamem_hip.mem] option --coverage-min-mapq needs a whole number, 0 .. 255", file=sys.stderr)
                return 2
            cov_mapq = int(argv[i + 1])
            i += 1
        elif a == "--coverage-deletions":
            cov_del = True
        elif a == "--rg":
            if i + 1 >= len(argv):
                print("[bwamem_hip.mem] option --rg needs a value", file=sys.stderr)
                return 2
            groups.append([argv[i + 1]])
            i += 1
        elif a in ("-o", "--device", "--index", "--sort-mem", "--sort-tmp", "--markdup-metrics"):
            if i + 1 >= len(argv):
                print(f"[bwamem_hip.mem] option {a} needs a value", file=sys.stderr)
                return 2
            if a == "-o":
                out_path = argv[i + 1]
            elif a == "--index":
                index_path = argv[i + 1]
            elif a == "--markdup-metrics":
                metrics_path = argv[i + 1]
            elif a == "--sort-tmp":
                sort_tmp = argv[i + 1]
            elif a == "--sort-mem":
                if not argv[i + 1].isdigit() or int(argv[i + 1]) < 1:
                    print("[bwamem_hip.mem] option --sort-mem needs a number of bytes", file=sys.stderr)
                    return 2
                sort_mem = int(argv[i + 1])
            else:
                device = argv[i + 1]
            i += 1
        elif a in FLAGS:
            opts.append(a)
        elif a.startswith("-") and len(a) > 1:
            if a not in VALUED:
                print(f"[bwamem_hip.mem] option {a} is not taken", file=sys.stderr)
                return 2
            if i + 1 >= len(argv):
                print(f"[bwamem_hip.mem] option {a} needs a value", file=sys.stderr)
                return 2
            opts += [a, argv[i + 1]]
            i += 1
        elif groups:
            groups[-1].append(a)
        else:
            pos.append(a)
        i += 1
    if keep_rg and (groups or "-R" in opts):
        print("[bwamem_hip.mem] --keep-rg excludes --rg and -R: the read groups come from the input BAM's own header and tags, or from the command line, not both", file=sys.stderr)
        return 2
    if collate_mem is not None and not collate:
        print("[bwamem_hip.mem] --collate-mem needs --collate (it caps the records that wait for their mates)", file=sys.stderr)
        return 2
    if groups:
        if "-R" in opts:
            print("[bwamem_hip.mem] --rg and -R exclude each other: with --rg every group brings its own @RG line", file=sys.stderr)
            return 2
        if len(pos) > 1:
            print(f"[bwamem_hip.mem] read files before the first --rg ({pos[1]}): with --rg every read file follows its group's --rg", file=sys.stderr)
            return 2
        for g in groups:
            if len(g) not in (2, 3):
                print(f"[bwamem_hip.mem] --rg {g[0]!r} is followed by {len(g) - 1} files: a group is one file of reads, or reads and mates", file=sys.stderr)
                return 2
        if len(pos) != 1:
            print(__doc__, file=sys.stderr)
            return 2
    elif len(pos) not in (2, 3):
        print(__doc__, file=sys.stderr)
        return 2
    prefix, reads, mates = pos[0], pos[1] if len(pos) > 1 else None, pos[2] if len(pos) == 3 else None
    if not sort and (index_path is not None or sort_mem is not None or sort_tmp is not None):
        print("[bwamem_hip.mem] --index, --sort-mem and --sort-tmp need --sort", file=sys.stderr)
        return 2
    if markdup and not sort:
        print("[bwamem_hip.mem] --markdup needs --sort", file=sys.stderr)
        return 2
    if metrics_path is not None and not markdup:
        print("[bwamem_hip.mem] --markdup-metrics needs --markdup", file=sys.stderr)
        return 2
    if optical is not None and not markdup:
        print("[bwamem_hip.mem] --optical-distance needs --markdup (optical duplicates are counted where duplicates are marked)", file=sys.stderr)
        return 2
    if barcode_edits is not None and not markdup:
        print("[bwamem_hip.mem] --barcode-edits needs --markdup (barcodes are grouped where duplicates are marked)", file=sys.stderr)
        return 2
    if barcode_edits is not None and barcode_tag is None and not barcode_name:
        print("[bwamem_hip.mem] --barcode-edits needs --barcode-tag or --barcode-name (it groups the barcodes that are compared)", file=sys.stderr)
        return 2
    if barcode_tag is not None or barcode_name:
        from .lib import barcode_source
        try:
            barcode_source(barcode_tag, barcode_name or None, "--barcode-tag")
        except ValueError as e:
            print(f"[bwamem_hip.mem] {e}", file=sys.stderr)
            return 2
        if not markdup:
            print("[bwamem_hip.mem] --barcode-tag and --barcode-name need --markdup (barcodes are compared where duplicates are marked)", file=sys.stderr)
            return 2
        if barcode_tag is not None and "-C" not in opts:
            print("[bwamem_hip.mem] --barcode-tag needs -C: the tag reaches a record only as the read's comment", file=sys.stderr)
            return 2
    if (cov_paths or cov_bin is not None or cov_mapq is not None or cov_del) and not sort:
        print("[bwamem_hip.mem] --coverage, --coverage-hist, --coverage-bed, --coverage-bin, --coverage-min-mapq and --coverage-deletions need --sort (depth is computed where the sorted file is written)", file=sys.stderr)
        return 2
    if (recal_sites or "recal_min_qual" in recal_kw or "recal_max_cycle" in recal_kw) and "recal" not in recal_kw:
        print("[bwamem_hip.mem] --known-sites, --recal-min-qual and --recal-max-cycle need --recal (they say what is counted, not where it goes)", file=sys.stderr)
        return 2
    if recal_kw and not sort:
        print("[bwamem_hip.mem] --recal, --known-sites, --recal-min-qual and --recal-max-cycle need --sort (the table is counted where the sorted file is written)", file=sys.stderr)
        return 2
    if "apply_recal_report" in apply_kw and "apply_recal" not in apply_kw:
        print("[bwamem_hip.mem] --apply-recal-report needs --apply-recal (it says what the applied table changed)", file=sys.stderr)
        return 2
    if apply_kw and not sort:
        print("[bwamem_hip.mem] --apply-recal and --apply-recal-report need --sort (the qualities are rewritten where the sorted file is written)", file=sys.stderr)
        return 2
    if "apply_recal" in apply_kw:
        if "recal" in recal_kw and os.path.abspath(recal_kw["recal"]) == os.path.abspath(apply_kw["apply_recal"]):
            print("[bwamem_hip.mem] --recal and --apply-recal name the same file: counting and applying one table in one run would take two passes over the windows", file=sys.stderr)
            return 2
        from .recal import read_recal_table
        try:                                                      # (read before the output is opened: a file that is no table leaves nothing behind)
            apply_kw["apply_recal"] = read_recal_table(apply_kw["apply_recal"])
        except (ValueError, OSError) as e:
            print(f"[bwamem_hip.mem] --apply-recal: {e}", file=sys.stderr)
            return 1
    if stats_paths and not sort:
        print("[bwamem_hip.mem] --flagstat, --idxstats and --stats need --sort (the statistics are computed where the sorted file is written)", file=sys.stderr)
        return 2
    if ("--coverage-bed" in cov_paths) != (cov_bin is not None):
        print("[bwamem_hip.mem] --coverage-bed and --coverage-bin go together (the bins of the BED file)", file=sys.stderr)
        return 2
    if (cov_mapq is not None or cov_del) and not cov_paths:
        print("[bwamem_hip.mem] --coverage-min-mapq and --coverage-deletions need --coverage, --coverage-hist or --coverage-bed (they say what is counted, not where it goes)", file=sys.stderr)
        return 2
    if csi_shift is not None and not csi:
        print("[bwamem_hip.mem] --csi-min-shift needs --csi (a BAI index has one bin size)", file=sys.stderr)
        return 2
    if sort and index_path is None and out_path is not None:
        index_path = out_path + (".csi" if csi else ".bai")
    from .aligner import Aligner
    try:
        al = Aligner(prefix, device=device, long_reads=long_reads)
        al.set_options(opts)
    except (OSError, ValueError) as e:
        print(f"[bwamem_hip.mem] {e}", file=sys.stderr)
        return 1
    out = open(out_path, "wb") if out_path is not None else sys.stdout.buffer
    try:
        paired = interleaved or mates is not None
        fmt_kw = dict(fmt="bam", level=bam_level) if bam else {}
        if sort:
            fmt_kw.update(sort=True, index=index_path, sort_mem=sort_mem, sort_tmp=sort_tmp)
        if markdup:
            fmt_kw.update(markdup=True, markdup_metrics=metrics_path)
        if optical is not None:
            fmt_kw.update(optical_distance=optical)
        if barcode_tag is not None:
            fmt_kw.update(barcode_tag=barcode_tag)
        if barcode_name:
            fmt_kw.update(barcode_name=True)
        if barcode_edits is not None:
            fmt_kw.update(barcode_edits=barcode_edits)
        if csi:
            fmt_kw.update(index_format="csi", csi_min_shift=14 if csi_shift is None else csi_shift)
        if collate:
            fmt_kw.update(collate=True, collate_mem=collate_mem)
        if cov_paths:
            fmt_kw.update(coverage=cov_paths.get("--coverage"), coverage_hist=cov_paths.get("--coverage-hist"), coverage_bed=cov_paths.get("--coverage-bed"), coverage_bin=cov_bin,
                          coverage_min_mapq=cov_mapq, coverage_deletions=cov_del)
        if stats_paths:
            fmt_kw.update(flagstat=stats_paths.get("--flagstat"), idxstats=stats_paths.get("--idxstats"), stats=stats_paths.get("--stats"))
        if recal_kw:
            fmt_kw.update(recal_kw, known_sites=recal_sites or None)
        if apply_kw:
            fmt_kw.update(apply_kw)
        done = False
        if groups:
            al.align_groups([(g[0], g[1], g[2] if len(g) == 3 else None) for g in groups], out=out, paired=interleaved, **fmt_kw)
            done = True
        elif mates is None and _plain_regular(reads) and not keep_rg and not collate:
            from .lib import ReadFileError
            try:
                al.align_file(reads, out, paired=paired, **fmt_kw)
                done = True
            except ReadFileError:                                    # (its counting pass refused the layout: nothing has been written)
                pass
        if not done:
            al.align_files(reads, mates, out=out, paired=paired, **fmt_kw, **(dict(keep_rg=True) if keep_rg else {}))
        out.flush()
    except (ValueError, NotImplementedError) as e:
        print(f"[bwamem_hip.mem] {e}", file=sys.stderr)
        return 1
    finally:
        if out_path is not None:
            out.close()
        al.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
