"""Sort, mark duplicates and index a BAM or SAM that any aligner wrote, on the device.

    python -m bwamem_hip.bam [options] IN [-o OUT.bam]

IN is a BAM file or SAM text (plain, gzip or BGZF; a regular file, a pipe, or - for stdin; told apart by their bytes) from `bwa mem`, bwa-mem2, minimap2, bowtie2 or
`python -m bwamem_hip.mem` without --sort.  No index prefix is needed.  The output is the coordinate-sorted BAM (-o; default stdout) with its index: with -o PATH
the index goes to PATH.bai (PATH.csi with --csi), --index PATH names it otherwise, and on stdout without --index none is written.  The header is the input's with
its @HD line replaced by `@HD VN:1.6 SO:coordinate`; no @PG line is added.  Records stay verbatim but for the bin (recomputed) and, with --markdup, flag 0x400.

The options are those of bwamem_hip.mem, with the same meaning and the same refusals: --markdup, --markdup-metrics PATH, --optical-distance N, --barcode-tag XX,
--barcode-name, --barcode-edits N; --coverage PATH, --coverage-hist PATH, --coverage-bed PATH, --coverage-bin N, --coverage-min-mapq Q, --coverage-deletions; --flagstat PATH, --idxstats PATH, --stats PATH; --recal PATH with --reference PREFIX, --known-sites FILE (repeatable), --recal-min-qual Q, --recal-max-cycle N;
--apply-recal TABLE, --apply-recal-report PATH (they need no --reference, and --host works);
--csi, --csi-min-shift N, --index PATH, --bam-level 0|1, --sort-mem BYTES, --sort-tmp DIR, --sort-window RECORDS.  Here --barcode-tag needs no -C: the tag is read
from the record.  Beside them: --libraries (needs --markdup: the header's @RG lines are the table of libraries, duplicates are called within a library and the
metrics table has a row per library; the rules and refusals of `bwamem_hip.mem --keep-rg --markdup`; off: one library), --batch-bytes N (the record bytes of a
sorted run; 256 MiB, at most 1 GiB; no output depends on it), --host (the host forms of every step: no device is needed, and the whole record stream is held in
memory) and --device (the torch device, cuda:0).

--markdup alone needs the records of a read name next to each other, in any order -- what every aligner writes.  A file that has them apart, such as a
coordinate-sorted one, takes --markdup --collate: templates are then the records of the whole file under one read name, adjacent or not, numbered by their first
records (BDP_TPL_FILE).  --collate needs --markdup, works with every other option, and keeps 32 bytes per record in host memory (48 / 56 with
--optical-distance / barcodes) until the last batch is in; a name whose records are no proper template -- a pair without exactly one 0x40 and one 0x80 primary
line, two templates under one name -- is refused by the index of its first record.  On a name-grouped file with distinct names the output is that without it.
Without --collate such a file is sorted and indexed without --markdup and refused with it.  A refused input ends the command with status 1 and the library's
message on stderr.
"""
from __future__ import annotations

import os
import sys


def bam_post_file(src, out, index=None, host: bool = False, level: int = 1, sort_window: int = 0, sort_mem=None, sort_tmp=None, batch_bytes=None, index_format: str = "bai",
                  csi_min_shift: int = 14, markdup: bool = False, markdup_metrics=None, libraries: bool = False, optical_distance=None, barcode_tag=None, barcode_name=None,
                  barcode_edits=None, coverage=None, coverage_hist=None, coverage_bed=None, coverage_bin=None, coverage_min_mapq=None, coverage_deletions=False, collate: bool = False,
                  flagstat=None, idxstats=None, stats=None, insert_cap=None, recal=None, reference=None, known_sites=None, recal_min_qual=None, recal_max_cycle=None, apply_recal=None, apply_recal_report=None) -> dict:
    """the BAM or SAM file `src` (a path; "-": stdin) -> the coordinate-sorted BAM written to `out` (a binary file object), its index to `index` (a path or a binary
    file object; None: not written), the metrics table to `markdup_metrics` and the coverage texts to coverage / coverage_hist / coverage_bed (paths or text file
    objects), as Aligner.align_files(sort=True, ...) writes them.  Returns lib.bam_post's dict.  The keywords are align_files' and are refused as there.
    collate=True (needs markdup=True): templates by name over the whole file, for an input that is not grouped by name (lib.bam_post).
    flagstat / idxstats / stats (paths or text file objects) and insert_cap: align_files' -- the statistics of the sorted file, from the windows of its merge.
    apply_recal (a path to a table recal wrote, or read_recal_table's dict; needs no reference): the base qualities are recalibrated by that table as the sorted file
    is written (align_files' keyword), apply_recal_report (a path or a text file object) takes recal_apply_report_text's rows; "recal_apply" holds the counts.
    recal (a path or a text file object; needs reference=PREFIX): the recalibration table of the sorted file against PREFIX.pac / .ann / .amb, under
    known_sites (VCF or BED files), recal_min_qual and recal_max_cycle; its read groups are the header's @RG lines (none: the one group `*`).  `src` is read twice --
    its header first -- so it is a file, not a pipe; a header whose @SQ lines are not the .ann's names and lengths in order is refused before anything is written."""
    from .aligner import recal_request, stats_request, write_stats_texts
    from .aligner import coverage_request, coverage_table_text, coverage_hist_text, coverage_bed_text, markdup_metrics_text, markdup_metrics_text_libraries, _write_text
    from .lib import bam_post
    if not ("b" in getattr(out, "mode", "") or hasattr(out, "getbuffer")):
        raise ValueError("bam_post_file: the output needs a binary file object")
    if markdup_metrics is not None and not markdup:
        raise ValueError("bam_post_file: markdup_metrics needs markdup=True")
    req = coverage_request("bam_post_file", True, coverage, coverage_hist, coverage_bed, coverage_bin, coverage_min_mapq, coverage_deletions)
    sreq = stats_request("bam_post_file", True, flagstat, idxstats, stats, insert_cap)
    rreq = recal_request("bam_post_file", reference is not None, recal, known_sites, recal_min_qual, recal_max_cycle, apply_recal, apply_recal_report, need="reference=PREFIX")
    if (rreq is None or rreq["table"] is None) and reference is not None:
        raise ValueError("bam_post_file: reference needs recal (the reference is read for the recalibration table alone)")
    recal_kw = None if rreq is None or rreq["table"] is None else _recal_keywords(src, reference, rreq)
    if rreq is not None and rreq["apply"] is not None:             # the table applied to the qualities as they are written; alone, no table is counted and no reference read
        recal_kw = dict(recal_kw, apply=rreq["apply"]) if recal_kw is not None else dict(apply=rreq["apply"], count=False)
    r = bam_post("/dev/stdin" if src == "-" else src, out.write, host=host, level=level, window=sort_window, index_format=index_format, csi_min_shift=csi_min_shift, sort_mem=sort_mem,
                 sort_tmp=sort_tmp, batch_bytes=batch_bytes, markdup=markdup, libraries=libraries, optical_distance=optical_distance, barcode_tag=barcode_tag, barcode_name=barcode_name,
                 barcode_edits=barcode_edits, coverage=None if req is None else dict(min_mapq=req["min_mapq"], deletions=req["deletions"], bin=req["bin"]), collate=collate,
                 stats=None if sreq is None else dict(insert_cap=sreq["insert_cap"]), recal=recal_kw)
    if index is not None:
        if hasattr(index, "write"):
            index.write(r["index"])
        else:
            with open(index, "wb") as f:
                f.write(r["index"])
    if req is not None:
        if req["table"] is not None:
            _write_text(req["table"], coverage_table_text(r["coverage"], r["contigs"]))
        if req["hist"] is not None:
            _write_text(req["hist"], coverage_hist_text(r["coverage"]))
        if req["bed"] is not None:
            _write_text(req["bed"], coverage_bed_text(r["coverage"], r["contigs"], req["bin"]))
    if sreq is not None:
        write_stats_texts(sreq, r["stats"], r["contigs"])
    if rreq is not None and rreq["apply"] is not None:
        r["recal_apply"] = r["recal"].pop("apply")
        if rreq["apply_report"] is not None:
            from .recal import write_recal_apply_report
            write_recal_apply_report(r["recal_apply"], rreq["apply_report"])
    if rreq is not None and rreq["table"] is not None:
        from .recal import write_recal_table
        write_recal_table(r["recal"], rreq["table"])
    if markdup_metrics is not None:
        _write_text(markdup_metrics, markdup_metrics_text_libraries(r["markdup"]["libraries"]) if libraries else markdup_metrics_text(r["markdup"]))
    return r


def peek_header(src: str):
    """the header of the BAM or SAM file at `src` (plain, gzip or BGZF), read ahead of the run: (its text, its contigs as (name, length) pairs)"""
    import gzip
    import struct
    with open(src, "rb") as f:
        zipped = f.read(2) == b"\x1f\x8b"
    with (gzip.open if zipped else open)(src, "rb") as f:
        if f.read(4) == b"BAM\1":
            text = f.read(struct.unpack("<I", f.read(4))[0]).split(b"\0")[0].decode("latin-1")
            contigs = []
            for _ in range(struct.unpack("<I", f.read(4))[0]):
                name = f.read(struct.unpack("<I", f.read(4))[0])[:-1].decode("latin-1")
                contigs.append((name, struct.unpack("<I", f.read(4))[0]))
            return text, contigs
        f.seek(0)
        lines = []
        for ln in f:
            if not ln.startswith(b"@"):
                break
            lines.append(ln.decode("latin-1"))
    contigs = []
    for ln in lines:
        if ln.startswith("@SQ"):
            tags = dict(x.split(":", 1) for x in ln.rstrip("\r\n").split("\t")[1:] if ":" in x)
            contigs.append((tags.get("SN", ""), int(tags.get("LN", "0"))))
    return "".join(lines), contigs


def _recal_keywords(src, reference: str, rreq: dict) -> dict:
    """lib.bam_post's recal keyword for a run over `src` against the reference files at `reference`: the .pac body, the mask of the known sites and the .amb's
    holes, the header's read groups.  Refused before anything is written: a pipe, a header whose contigs are not the .ann's in order, more than 255 groups"""
    import numpy as np
    from .aligner import bam_read_groups, read_amb, read_ann
    from .lib import known_sites_mask
    if src == "-":
        raise ValueError("bam_post_file: recal reads the input's header before the run: a file, not a pipe")
    contigs, l_pac = read_ann(reference)
    text, have = peek_header(src)
    if have != contigs:
        k = next((i for i, (a, b) in enumerate(zip(have, contigs)) if a != b), min(len(have), len(contigs)))
        raise ValueError(f"bam_post_file: the input's @SQ lines are not {reference}.ann's names and lengths in order ({len(have)} against {len(contigs)} contigs; the first that differs is number {k})")
    groups = [g[1] for g in bam_read_groups(text)] if any(ln.startswith("@RG") for ln in text.split("\n")) else None
    if groups is not None and len(groups) > 255:
        raise ValueError(f"bam_post_file: {len(groups)} read groups: the recalibration table holds at most 255")
    pac = np.fromfile(reference + ".pac", dtype=np.uint8)[:(l_pac + 3) // 4]
    mask = known_sites_mask(rreq["known_sites"], contigs, l_pac=l_pac, holes=read_amb(reference))
    return dict(pac=pac, l_pac=l_pac, mask=mask, read_groups=groups, min_qual=rreq["min_qual"], max_cycle=rreq["max_cycle"], known_sites=rreq["known_sites"])


_VALUED = ("-o", "--device", "--index", "--sort-mem", "--sort-tmp", "--sort-window", "--markdup-metrics", "--batch-bytes", "--coverage", "--coverage-hist", "--coverage-bed", "--barcode-tag", "--flagstat", "--idxstats", "--stats",
           "--bam-level", "--csi-min-shift", "--optical-distance", "--barcode-edits", "--coverage-bin", "--coverage-min-mapq", "--recal", "--reference", "--recal-min-qual", "--recal-max-cycle", "--apply-recal", "--apply-recal-report")
_NUMBERS = {"--bam-level": (0, 1, "0 or 1"), "--csi-min-shift": (10, 24, "a number in 10 .. 24"), "--optical-distance": (0, 0x7fffffff, "a whole number of pixels, 0 .. 2^31 - 1"),
            "--barcode-edits": (0, 21, "a whole number of mismatches, 0 .. 21"), "--coverage-bin": (1, 0xffffffff, "a whole number of positions, 1 .. 2^32 - 1"),
            "--coverage-min-mapq": (0, 255, "a whole number, 0 .. 255"), "--sort-mem": (1, 1 << 62, "a number of bytes"), "--batch-bytes": (1, 1 << 30, "a number of bytes, at most 2^30"),
            "--sort-window": (1, 0xffffffff, "a number of records"), "--recal-min-qual": (0, 93, "a quality, 0 .. 93"), "--recal-max-cycle": (1, 65535, "a number of cycles, 1 .. 65535")}


def main(argv=None) -> int:
    argv = list(sys.argv[1:] if argv is None else argv)
    me = "[bwamem_hip.bam]"
    v, flags, pos, sites = {}, set(), [], []
    i = 0
    while i < len(argv):
        a = argv[i]
        if a in ("--markdup", "--barcode-name", "--coverage-deletions", "--csi", "--libraries", "--host", "--collate"):
            flags.add(a)
        elif a == "--known-sites":                                 # (repeatable)
            if i + 1 >= len(argv):
                print(f"{me} option {a} needs a value", file=sys.stderr)
                return 2
            sites.append(argv[i + 1])
            i += 1
        elif a in _VALUED:
            if i + 1 >= len(argv):
                print(f"{me} option {a} needs a value", file=sys.stderr)
                return 2
            val = argv[i + 1]
            if a in _NUMBERS:
                lo, hi, words = _NUMBERS[a]
                if not (val.isascii() and val.isdigit()) or not lo <= int(val) <= hi:
                    print(f"{me} option {a} needs {words}", file=sys.stderr)
                    return 2
                val = int(val)
            v[a] = val
            i += 1
        elif a.startswith("-") and len(a) > 1:
            print(f"{me} option {a} is not taken", file=sys.stderr)
            return 2
        else:
            pos.append(a)
        i += 1
    if len(pos) != 1:
        print(__doc__, file=sys.stderr)
        return 2
    markdup = "--markdup" in flags
    cov_paths = {k: v[k] for k in ("--coverage", "--coverage-hist", "--coverage-bed") if k in v}
    checks = [("--markdup-metrics" in v and not markdup, "--markdup-metrics needs --markdup"),
              ("--optical-distance" in v and not markdup, "--optical-distance needs --markdup (optical duplicates are counted where duplicates are marked)"),
              ("--barcode-edits" in v and not markdup, "--barcode-edits needs --markdup (barcodes are grouped where duplicates are marked)"),
              ("--barcode-edits" in v and "--barcode-tag" not in v and "--barcode-name" not in flags, "--barcode-edits needs --barcode-tag or --barcode-name (it groups the barcodes that are compared)"),
              ("--collate" in flags and not markdup, "--collate needs --markdup (templates by name over the whole file are formed where duplicates are marked)"),
              ("--libraries" in flags and not markdup, "--libraries needs --markdup (the libraries say which templates may be duplicates of each other)"),
              (("--coverage-bed" in cov_paths) != ("--coverage-bin" in v), "--coverage-bed and --coverage-bin go together (the bins of the BED file)"),
              (("--coverage-min-mapq" in v or "--coverage-deletions" in flags) and not cov_paths,
               "--coverage-min-mapq and --coverage-deletions need --coverage, --coverage-hist or --coverage-bed (they say what is counted, not where it goes)"),
              ("--csi-min-shift" in v and "--csi" not in flags, "--csi-min-shift needs --csi (a BAI index has one bin size)"),
              ((sites or "--recal-min-qual" in v or "--recal-max-cycle" in v) and "--recal" not in v,
               "--known-sites, --recal-min-qual and --recal-max-cycle need --recal (they say what is counted, not where it goes)"),
              ("--recal" in v and "--reference" not in v, "--recal needs --reference PREFIX (the table compares the reads with PREFIX.pac, .ann and .amb)"),
              ("--reference" in v and "--recal" not in v, "--reference needs --recal (the reference is read for the recalibration table alone)"),
              ("--apply-recal-report" in v and "--apply-recal" not in v, "--apply-recal-report needs --apply-recal (it says what the applied table changed)"),
              ("--apply-recal" in v and "--recal" in v and os.path.abspath(v["--apply-recal"]) == os.path.abspath(v["--recal"]),
               "--recal and --apply-recal name the same file: counting and applying one table in one run would take two passes over the windows")]
    for bad, words in checks:
        if bad:
            print(f"{me} {words}", file=sys.stderr)
            return 2
    if "--barcode-tag" in v or "--barcode-name" in flags:
        from .lib import barcode_source
        try:
            barcode_source(v.get("--barcode-tag"), True if "--barcode-name" in flags else None, "--barcode-tag")
        except ValueError as e:
            print(f"{me} {e}", file=sys.stderr)
            return 2
        if not markdup:
            print(f"{me} --barcode-tag and --barcode-name need --markdup (barcodes are compared where duplicates are marked)", file=sys.stderr)
            return 2
    apply_table = None
    if "--apply-recal" in v:                                       # (read before the output is opened: a file that is no table leaves nothing behind)
        from .recal import read_recal_table
        try:
            apply_table = read_recal_table(v["--apply-recal"])
        except (ValueError, OSError) as e:
            print(f"{me} --apply-recal: {e}", file=sys.stderr)
            return 1
    out_path, csi, host = v.get("-o"), "--csi" in flags, "--host" in flags
    index_path = v.get("--index")
    if index_path is None and out_path is not None:
        index_path = out_path + (".csi" if csi else ".bai")
    if not host:
        import torch
        torch.cuda.set_device(torch.device(v.get("--device", "cuda:0")))
    out = open(out_path, "wb") if out_path is not None else sys.stdout.buffer
    try:
        bam_post_file(pos[0], out, index=index_path, host=host, level=v.get("--bam-level", 1), sort_window=v.get("--sort-window", 0), sort_mem=v.get("--sort-mem"), sort_tmp=v.get("--sort-tmp"),
                      batch_bytes=v.get("--batch-bytes"), index_format="csi" if csi else "bai", csi_min_shift=v.get("--csi-min-shift", 14), markdup=markdup,
                      markdup_metrics=v.get("--markdup-metrics"), libraries="--libraries" in flags, optical_distance=v.get("--optical-distance"), barcode_tag=v.get("--barcode-tag"),
                      barcode_name=True if "--barcode-name" in flags else None, barcode_edits=v.get("--barcode-edits"), coverage=cov_paths.get("--coverage"),
                      coverage_hist=cov_paths.get("--coverage-hist"), coverage_bed=cov_paths.get("--coverage-bed"), coverage_bin=v.get("--coverage-bin"),
                      coverage_min_mapq=v.get("--coverage-min-mapq"), coverage_deletions="--coverage-deletions" in flags, collate="--collate" in flags,
                      flagstat=v.get("--flagstat"), idxstats=v.get("--idxstats"), stats=v.get("--stats"),
                      recal=v.get("--recal"), reference=v.get("--reference"), known_sites=sites or None, recal_min_qual=v.get("--recal-min-qual"), recal_max_cycle=v.get("--recal-max-cycle"),
                      apply_recal=apply_table, apply_recal_report=v.get("--apply-recal-report"))
        out.flush()
    except (ValueError, OSError) as e:
        print(f"{me} {e}", file=sys.stderr)
        return 1
    finally:
        if out_path is not None:
            out.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
