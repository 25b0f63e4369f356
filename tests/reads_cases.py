"""Hand-made read files for the device record parser (csrc/reads_parse.hip), its pump and its escape to the host walker (csrc/reads_io.cpp:
bmh_walk_record): one small text per rule the kernels decide from one or two bytes, each on both sides of its boundary.  Plain Python: no tests, no GPU,
no library import at module level.

  cases()      name -> (text, kind, route): kind "fa" / "fq"; route "device" when the kernels must take the whole file at the default window, "host"
               when at least one window must go to the walker.  What every text must parse to is recorded from the reference's kseq_read in
               tests/golden/reads_input/cases_expected.npz (scripts/record_reads_golden.py --cases).
  refusals()   name -> (text, piece of the walker's message)
  pairs()      name -> (text1, text2): two-file cases, interleaved as bseq_read interleaves them
  kseq_model   a literal restatement of kseq_read (src/kseq.h of the reference: ks_getc, ks_getuntil2, kseq_read) plus trim_readno (src/bwa.c), written
               from that header and not from the walker; model_outcome adds the refusals this project words where kseq_read gives up or returns an empty
               record
  device_route the flag rules of the header comment of csrc/reads_parse.hip restated for a whole file in one window: which route a text takes.  It is a
               statement about speed, never about what is parsed: the table's declared routes are checked against it on the CPU, and it sorts the
               random corpus into its two routes
  random_texts a seeded corpus joined from line pieces, for inputs no fixture holds

Routes that are not what one might expect, and why:
  a blank line inside a FASTQ record     device: the kernels count the non-empty lines four to a record, which is what kseq_read does with an empty line
                                         in front of the sequence, the '+' line or the qualities; only a lone CR there is kseq's to keep or drop
  leading "\r\n" lines before a FASTA    host: a lone CR that is not behind sequence bytes raises the flag wherever it stands (LK_LCR); in front of a
  header                                 FASTQ header it stands between records and stays on the device
  a last header line without its '\n'    kseq_read returns a record with an empty sequence, which the walker refuses: it is in refusals(), and the device
                                         reaches the message through its end-of-file flag"""
from __future__ import annotations

TAIL_FA = b">z\nGATTACA\n"
TAIL_FQ = b"@z\nGATTACA\n+\nIIHGFED\n"


class _Lcg:
    """a generator of our own, so that the table's bytes depend on no library's version"""

    def __init__(self, seed: int):
        self.s = (seed * 6364136223846793005 + 1442695040888963407) & 0xFFFFFFFFFFFFFFFF

    def next(self, n: int) -> int:
        self.s = (self.s * 6364136223846793005 + 1442695040888963407) & 0xFFFFFFFFFFFFFFFF
        return (self.s >> 33) % n

    def chance(self, per_thousand: int) -> bool:
        return self.next(1000) < per_thousand

    def pick(self, seq):
        return seq[self.next(len(seq))]


def bases(seed: int, n: int) -> bytes:
    g = _Lcg(seed)
    return bytes(b"ACGT"[g.next(4)] for _ in range(n))


def wrap(s: bytes, w: int, eol: bytes = b"\n") -> bytes:
    return b"".join(s[i:i + w] + eol for i in range(0, len(s), w))


def _fq(name: bytes, seq: bytes, qual: bytes, plus: bytes = b"+", eol: bytes = b"\n") -> bytes:
    return b"@" + name + eol + seq + eol + plus + eol + qual + eol


# ---------------------------------------------------------------------------------------------------------------- the table

def cases() -> dict:
    c = {}

    def fa(name, text, route="device"):
        assert name not in c
        c[name] = (text, "fa", route)

    def fq(name, text, route="device"):
        assert name not in c
        c[name] = (text, "fq", route)

    # ---- names: trim_readno's "/<digit>" with its length guard, the isspace byte that ends a name
    fa("name_slash1_len2", b">/1\nACGT\n" + TAIL_FA)                           # "/1" stays: the nl_ > 2 guard
    fa("name_slash1_len3", b">a/1\nACGT\n" + TAIL_FA)                          # -> "a"
    fa("name_slash1_len4", b">ab/1\nACGT\n>cd/2 x\nTTGA\n" + TAIL_FA)
    fa("name_slash_letter", b">ab/a\nACGT\n>ab/\nACGT\n>ab/:\nAC\n>ab//\nAC\n" + TAIL_FA)        # ':' and '/' sit next to the digits
    fa("name_slash12", b">ab/12\nACGT\n>/12\nAC\n>a/0\nAC\n>a/9\nAC\n" + TAIL_FA)
    fa("name_slash1_slash2", b">x/1/2\nACGT\n>x/1/\nAC\n>1/1\nAC\n" + TAIL_FA)
    fa("name_empty", b">\nACGT\n> only a comment\nAC\n" + TAIL_FA)
    for tag, sp in (("blank", b" "), ("tab", b"\t"), ("vt", b"\v"), ("ff", b"\f"), ("cr", b"\r")):
        fa("name_ends_" + tag, b">ab/1" + sp + b"c d\nACGT\n>e" + sp + b"\nAC\n" + TAIL_FA)
    fa("name_len1", b">a\nACGT\n>b\nAC\n")
    fa("name_len255", b">" + b"n" * 253 + b"/1 c\nACGT\n>" + b"m" * 100 + b"\nAC\n")
    fq("fq_names", _fq(b"/1", b"ACGT", b"IIII") + _fq(b"a/1", b"AC", b"II") + _fq(b"ab/2\tc", b"ACG", b"III") + _fq(b"", b"A", b"I") + _fq(b"x/1/2\vq", b"AC", b"II")
       + _fq(b"ab/a", b"AC", b"II") + _fq(b"q/12 \r", b"AC", b"II", eol=b"\r\n"))

    # ---- comments: kseq's rest of the header line, its trailing CR dropped only when the comment is longer than it
    fa("cm_none", b">a\nACGT\n" + TAIL_FA)
    fa("cm_empty", b">a \nACGT\n" + TAIL_FA)
    fa("cm_only_cr", b">a \r\nACGT\r\n" + TAIL_FA)                              # kept: the cl > 1 guard
    fa("cm_x_cr", b">a x\r\nACGT\r\n>b xy\r\nAC\r\n" + TAIL_FA)                   # CR dropped
    fa("cm_tabs_blanks", b">a\tx  y\t\tz \nACGT\n>b  \t two\nAC\n" + TAIL_FA)
    fa("cm_name_crlf", b">a\r\nACGT\r\n>bc\r\nAC\r\n")
    fa("cm_last_header", b">a\nAC\n>b the last one\tq\nGT\n")
    fq("fq_comments", _fq(b"a", b"AC", b"II") + _fq(b"b ", b"AC", b"II") + _fq(b"c \r", b"AC", b"II", eol=b"\r\n")[:-2] + b"\n" + _fq(b"d x", b"AC", b"II", eol=b"\r\n") + _fq(b"e\tx  y", b"AC", b"II"))

    # ---- FASTA sequence lines
    fa("fa_one_line", b">a c\nACGTACGTAC\n" + TAIL_FA)
    for w in (1, 2):
        fa(f"fa_width{w}", b">a\n" + wrap(bases(w, 7), w) + b">b\n" + wrap(bases(w + 10, 4), w))
    for w in (60, 61):
        fa(f"fa_width{w}", b">a c\n" + wrap(bases(w, 2 * w), w) + b">b\n" + wrap(bases(w + 10, w + 1), w) + TAIL_FA)           # whole lines, and a last line of one base
    fa("fa_short_last_line", b">a\n" + wrap(bases(5, 23), 10) + b">b\n" + wrap(bases(6, 11), 10))
    fa("fa_blank_lines", b">a\nACGT\n\nTTGA\n\n\nCC\n\n>b\n\nAC\n\n" + TAIL_FA + b"\n\n")
    fa("fa_crlf", b">a c\r\nACGT\r\nTTGA\r\nC\r\n>b\r\nAC\r\n")
    fa("fa_lone_cr_behind_seq", b">a\nACGT\n\r\nTTGA\n\r\n>b\r\nAC\r\n\r\n" + TAIL_FA)               # dropped by kseq: the sequence already holds bytes
    fa("fa_lone_cr_first_seq_line", b">a\n\r\nACGT\n" + TAIL_FA, "host")                      # kept by kseq as the record's first base
    fa("fa_lone_cr_behind_blank", b">a\nACGT\n\n\r\nTT\n" + TAIL_FA, "host")
    fa("fa_lone_cr_first_line", b"\r\n>a\nACGT\n" + TAIL_FA, "host")
    fa("fa_lone_cr_twice", b">a\r\nACGT\r\n\r\n\r\n>b\r\nAC\r\n", "host")
    fa("fa_last_no_nl", b">a\nACGT\n>b\nTTGAC")
    fa("fa_last_no_nl_one_base", b">a\nACGT\n>b\nTT\nG")
    fa("fa_last_ends_cr", b">a\nACGT\n>b\nTTGAC\r", "host")
    fa("fa_last_single_cr", b">a\nACGT\n>b\nTTGAC\n\r", "host")                      # kseq keeps it: the file ends before anything could be trimmed
    fa("fa_last_lone_gt", b">a\nACGT\n>b\nTTGAC\n>", "host")                         # makes no record
    fa("fa_codes", b">a\nacgtACGTnNrRyYkKmMsSwWbBdDhHvVuU\n>b\n*-.xX01\n" + TAIL_FA)
    fa("fa_blank_in_line", b">a\nAC GT\n A\nC \n" + TAIL_FA)

    # ---- FASTQ
    fq("fq_plus", _fq(b"a c", b"ACGT", b"IHGF") + _fq(b"b", b"TTGAC", b"FGHI#"))
    fq("fq_plus_name", _fq(b"a c", b"ACGT", b"IHGF", plus=b"+a c") + _fq(b"b", b"TTGAC", b"FGHI#", plus=b"+b") + _fq(b"d", b"AC", b"II", plus=b"+@d"))
    for tag, ch in (("at", b"@"), ("plus", b"+"), ("gt", b">")):
        for pos in range(4):
            recs = [_fq(b"r%d" % i, bases(30 + i, 3 + i), (ch + b"IHGFEDC")[:3 + i] if i == pos else b"ABCDEFG"[:3 + i]) for i in range(4)]
            fq(f"fq_qual_{tag}_rec{pos}", b"".join(recs))
    fq("fq_qual_all_at", b"".join(_fq(b"r%d x" % i, bases(40 + i, 2 + i), b"@" * (2 + i), plus=b"+r%d" % i) for i in range(4)))
    fq("fq_qual_is_a_header", _fq(b"a", b"ACG", b"@bc") + _fq(b"bc", b"AC", b"+@") + _fq(b"d", b"A", b">") + _fq(b"e", b"A", b"@") + _fq(b"f", b"A", b"+"))
    fq("fq_crlf", _fq(b"a c", b"ACGT", b"IHGF", eol=b"\r\n") + _fq(b"b", b"TTGAC", b"@GHI#", plus=b"+b", eol=b"\r\n"))
    fq("fq_blank_between", b"\n" + _fq(b"a", b"ACGT", b"IHGF") + b"\n\n" + _fq(b"b", b"TT", b"FG") + b"\n" + TAIL_FQ + b"\n\n")
    fq("fq_lone_cr_between", _fq(b"a", b"ACGT", b"IHGF", eol=b"\r\n") + b"\r\n" + _fq(b"b", b"TT", b"FG", eol=b"\r\n") + b"\r\n\r\n" + TAIL_FQ + b"\r\n")
    fq("fq_blank_inside", b"@a\n\nACGT\n+\nIHGF\n@b\nTT\n\n+\nFG\n@c\nAC\n+\n\nII\n" + TAIL_FQ)              # (device: see the module's comment)
    for k, where in enumerate(("seq", "plus", "qual")):
        # (kseq keeps the CR as the first base, drops it behind the bases, and keeps it as the first quality: the lengths are chosen to agree)
        lines = [b"@a", b"ACGT", b"+", (b"IHGFE", b"IHGF", b"IHG")[k]]
        lines.insert(k + 1, b"\r")
        fq("fq_lone_cr_before_" + where, b"".join(ln + b"\n" for ln in lines) + TAIL_FQ, "host")
    fq("fq_last_no_nl", _fq(b"a", b"ACGT", b"IHGF") + _fq(b"b", b"TT", b"FG")[:-1])
    fq("fq_last_ends_cr", _fq(b"a", b"ACGT", b"IHGF", eol=b"\r\n") + _fq(b"b", b"TT", b"FG", eol=b"\r\n")[:-1], "host")
    fq("fq_multi_line_seq", b"@a\nACGT\nTT\n+\nIHGFED\n" + TAIL_FQ, "host")
    fq("fq_multi_line_qual", b"@a\nACGTTT\n+\nIHGF\nED\n" + TAIL_FQ, "host")
    fq("fq_multi_line_both", b"@a\nACGT\nTT\nG\n+a\nIH\nGFE\nDC\n" + TAIL_FQ, "host")
    fq("fq_one_base", _fq(b"a", b"A", b"I") + _fq(b"b", b"C", b"@") + _fq(b"c", b"G", b"#", eol=b"\r\n"))

    # ---- leading bytes: both sides of the 64-byte peek of the device-inflate path
    for k in (0, 1, 63, 64, 65):
        fa(f"fa_lead_nl{k}", b"\n" * k + b">a c\nACGT\n" + TAIL_FA)
    for k in (63, 64, 65):
        fq(f"fq_lead_nl{k}", b"\n" * k + _fq(b"a c", b"ACGT", b"IHGF") + TAIL_FQ)
    fa("fa_lead_crlf", b"\r\n\r\n>a c\r\nACGT\r\n" + TAIL_FA, "host")
    fq("fq_lead_crlf", b"\r\n\r\n" + _fq(b"a c", b"ACGT", b"IHGF", eol=b"\r\n") + TAIL_FQ)
    fq("fq_lead_crlf33", b"\r\n" * 33 + _fq(b"a c", b"ACGT", b"IHGF", eol=b"\r\n") + TAIL_FQ)
    fa("fa_lead_text", b"some text\n>a c\nACGT\n" + TAIL_FA, "host")                # kseq skips to the first '>' / '@'
    fq("fq_lead_text", b"some text\n" + _fq(b"a c", b"ACGT", b"IHGF") + TAIL_FQ, "host")

    # ---- long lines: a window of 65 536 bytes and a BGZF member's 64 KiB boundary inside one record
    fa(LONG[0], b">long1 one line\n" + bases(71, 70_000) + b"\n" + TAIL_FA)
    fa(LONG[1], b">long2/1 sixty columns\n" + wrap(bases(72, 70_000), 60) + TAIL_FA)
    for name, (text, kind, route) in c.items():
        assert kind in ("fa", "fq") and route in ("device", "host") and (len(text) <= 400 or name in LONG), name
    return c


LONG = ("fa_long_line", "fa_long_60col")


def refusals() -> dict:
    """name -> (text, piece of bmh_walk_record's message)"""
    r = {}
    ok = _fq(b"a", b"ACGT", b"IHGF")
    r["fa_empty_seq"] = (b">a\n>b\nACGT\n", "empty sequence")
    r["fa_empty_seq_last"] = (b">a\nACGT\n>b\n", "empty sequence")
    r["fa_last_header_no_nl"] = (b">a\nACGT\n>b", "empty sequence")                 # kseq_read returns the empty record; see the module's comment
    r["fq_empty_seq"] = (b"@a\n\n+\n\n" + ok, "empty sequence")
    r["fq_empty_seq_second"] = (ok + b"@b\n+\n\n", "empty sequence")
    r["fq_qual_shorter"] = (b"@a\nACGT\n+\nIII\n@b\nAC\n+\nII\n", "quality line whose length differs")
    r["fq_qual_longer"] = (ok + b"@b\nACGT\n+\nIIIII\n@c\nAC\n+\nII\n", "quality line whose length differs")
    r["fq_qual_shorter_at_end"] = (ok + b"@b\nACGT\n+\nIII\n", "last record is truncated")
    r["fq_cut_after_header"] = (ok + b"@b\n", "FASTA and FASTQ records mixed")        # (to kseq_read a header and nothing else is a FASTA record)
    r["fq_cut_after_seq"] = (ok + b"@b\nACGT\n", "FASTA and FASTQ records mixed")
    r["fq_cut_after_plus"] = (ok + b"@b\nACGT\n+\n", "last record is truncated")
    r["fq_cut_in_plus"] = (ok + b"@b\nACGT\n+", "last record is truncated")
    r["fq_cut_in_qual"] = (ok + b"@b\nACGT\n+\nII", "last record is truncated")
    r["mixed_fq_then_fa"] = (ok + b">b\nACGT\n", "FASTA and FASTQ records mixed")
    r["mixed_fa_then_fq"] = (b">b\nACGT\n" + ok, "FASTA and FASTQ records mixed")
    r["fa_at_in_seq"] = (b">a\nAC\n@GT\n" + TAIL_FA, "empty sequence")                  # '@GT' is a header to kseq_read, without a sequence
    r["fa_plus_in_seq"] = (b">a\nAC\n+GT\n", "last record is truncated")               # '+GT' opens the qualities, and the file ends
    r["fa_plus_in_seq_then_fa"] = (b">a\nAC\n+\nII\n" + TAIL_FA, "FASTA and FASTQ records mixed")
    return r


def pairs() -> dict:
    """name -> (text1, text2)"""
    p = {}
    lens1, lens2 = (4, 1, 9, 6, 2), (7, 3, 1, 12, 5)
    r1 = [_fq(b"p%d/1 first" % i, bases(50 + i, n), bases(60 + i, n).replace(b"A", b"I").replace(b"C", b"@")) for i, n in enumerate(lens1)]
    r2 = [_fq(b"p%d/2\tsecond" % i, bases(70 + i, n), bases(80 + i, n).replace(b"A", b"#").replace(b"T", b"+"), plus=b"+p%d/2" % i, eol=b"\r\n") for i, n in enumerate(lens2)]
    p["pair_fq_lf_crlf"] = (b"".join(r1), b"".join(r2))
    p["pair_fq_blank_lines_in_2"] = (b"".join(r1), b"\n" + b"\n\n".join(r.replace(b"\r\n", b"\n") for r in r2) + b"\n")
    p["pair_fq_short_2"] = (b"".join(r1), b"".join(r2[:3]))
    p["pair_fq_short_1"] = (b"".join(r1[:2]), b"".join(r2))
    f1 = [b">q%d/1\n" % i + wrap(bases(90 + i, n), 5) for i, n in enumerate(lens2)]
    f2 = [b">q%d/2 m\r\n" % i + wrap(bases(95 + i, n), 3, b"\r\n") for i, n in enumerate(lens1)]
    p["pair_fa_multi_line"] = (b"".join(f1), b"".join(f2))
    p["pair_fa_short_2"] = (b"".join(f1), b"".join(f2[:4])[:-2])
    return p


SHORT_PAIRS = {"pair_fq_short_2": (1, 3), "pair_fq_short_1": (0, 2), "pair_fa_short_2": (1, 4)}      # name -> (the file that ends first, complete pairs)


# ---------------------------------------------------------------------------------------------------------------- kseq_read, restated

class Refusal(Exception):
    """what this project refuses with a message where kseq_read returns -2 (bseq_read ends the run silently) or an empty record; .piece is in the message"""

    def __init__(self, piece, records):
        super().__init__(piece)
        self.piece, self.records = piece, records


class _Stream:
    """kstream_t over the whole text: the 16 KiB buffer of the original changes nothing that is returned"""

    def __init__(self, text: bytes):
        self.t, self.p = text, 0

    def getc(self) -> int:                                # ks_getc
        if self.p >= len(self.t):
            return -1
        self.p += 1
        return self.t[self.p - 1]

    def getuntil(self, line: bool, s: bytearray, append: bool):
        """ks_getuntil2 with KS_SEP_LINE (line) or KS_SEP_SPACE: (its return value, the delimiter met or 0)"""
        if not append:
            del s[:]
        if self.p >= len(self.t):
            return -1, 0                                  # !gotany && ks_eof: nothing is trimmed
        i = self.p
        if line:
            while i < len(self.t) and self.t[i] != 10:
                i += 1
        else:
            while i < len(self.t) and not (self.t[i] == 32 or 9 <= self.t[i] <= 13):
                i += 1
        s += self.t[self.p:i]
        dret = self.t[i] if i < len(self.t) else 0
        self.p = i + 1 if i < len(self.t) else len(self.t)
        if line and len(s) > 1 and s[-1] == 13:
            del s[-1]
        return len(s), dret


def kseq_records(text: bytes):
    """kseq_read until it returns below 0: ([(name, comment, seq, qual, whether a '+' line followed the sequence)], that return value, whether the
    qualities ran into the end of the file)"""
    ks, last_char, out = _Stream(text), 0, []
    while True:
        if last_char == 0:                                # jump to the next header line
            c = ks.getc()
            while c != -1 and c != 62 and c != 64:
                c = ks.getc()
            if c == -1:
                return out, -1, False
            last_char = c
        name, comment, seq, qual = bytearray(), bytearray(), bytearray(), bytearray()
        ret, c = ks.getuntil(False, name, False)
        if ret < 0:
            return out, -1, False
        if c != 10:
            ks.getuntil(True, comment, False)
        c = ks.getc()
        while c != -1 and c != 62 and c != 43 and c != 64:
            if c != 10:                                   # (empty lines are skipped)
                seq.append(c)
                ks.getuntil(True, seq, True)              # the rest of the line
            c = ks.getc()
        if c == 62 or c == 64:
            last_char = c
        if c != 43:
            out.append((bytes(name), bytes(comment), bytes(seq), b"", False))
            continue                                      # (at the end of the file last_char stays set, and the next name is the -1 above)
        c = ks.getc()
        while c != -1 and c != 10:                        # the rest of the '+' line
            c = ks.getc()
        if c == -1:
            return out, -2, True
        ret, _ = ks.getuntil(True, qual, True)
        while ret >= 0 and len(qual) < len(seq):
            ret, _ = ks.getuntil(True, qual, True)
        last_char = 0
        if len(seq) != len(qual):
            return out, -2, ret < 0
        out.append((bytes(name), bytes(comment), bytes(seq), bytes(qual), True))


def trim_readno(name: bytes) -> bytes:
    return name[:-2] if len(name) > 2 and name[-2] == 47 and 48 <= name[-1] <= 57 else name


def kseq_model(text: bytes) -> list:
    """the records bseq_read makes of the text, (name, comment, seq, qual): kseq_read's, their names through trim_readno.  Raises Refusal where this
    project refuses the file -- in the order of the records, and for one record its qualities first, then its kind, then an empty sequence"""
    recs, ret, at_end = kseq_records(text)
    out, kind = [], 0
    for name, comment, seq, qual, plus in recs:
        k = 2 if plus else 1
        if kind and k != kind:
            raise Refusal("FASTA and FASTQ records mixed", out)
        kind = k
        if not seq:
            raise Refusal("empty sequence", out)
        out.append((trim_readno(name), comment, seq, qual))
    if ret == -2:
        raise Refusal("last record is truncated" if at_end else "quality line whose length differs", out)
    return out


def model_outcome(text: bytes):
    """("ok", records) or ("refused", message piece)"""
    try:
        return "ok", kseq_model(text)
    except Refusal as e:
        return "refused", e.piece


def pair_model(text1: bytes, text2: bytes):
    """bseq_read on two files: (the reads 2i, 2i+1 of the complete pairs, the file that ends first or None)"""
    a, b = kseq_model(text1), kseq_model(text2)
    n = min(len(a), len(b))
    return [r for pr in zip(a[:n], b[:n]) for r in pr], (None if len(a) == len(b) else 0 if len(a) < len(b) else 1)


def packed(records) -> dict:
    """the fields of cases_expected.npz for these records, as bytes and a list"""
    return dict(names=b"".join(r[0] + b"\0" for r in records), comments=b"".join(r[1] + b"\0" for r in records), seq=b"".join(r[2] for r in records),
                qual=b"".join(r[3] for r in records), lens=[len(r[2]) for r in records])


# ---------------------------------------------------------------------------------------------------------------- the route of a whole file

def device_route(text: bytes) -> str:
    """"device" when no rule of the header comment of csrc/reads_parse.hip raises the flag for the text as one window that ends the file, else "host\""""
    n = len(text)
    p = 0
    while p < n and text[p] in (10, 13):
        p += 1
    if p < n and text[p] not in (62, 64):
        return "host"                                     # text before the first header
    is_fq = p < n and text[p] == 64
    lines = text.split(b"\n")
    last_has_nl = text.endswith(b"\n")
    if last_has_nl:
        lines.pop()
    if not lines:
        return "device"

    def kind(c):
        return "blank" if not c else "lcr" if c == b"\r" else {62: ">", 64: "@", 43: "+"}.get(c[0], "seq")

    def klen(c):
        return len(c) - 1 if c.endswith(b"\r") else len(c)
    kinds = [kind(c) for c in lines]
    if not last_has_nl and (lines[-1].endswith(b"\r") or (not is_fq and kinds[-1] == ">")):
        return "host"                                     # the file's last line, unfinished: a header, or one that ends in CR
    if not is_fq:
        seen, length = False, 0
        for j, (c, k) in enumerate(zip(lines, kinds)):
            if k in ("@", "+"):
                return "host"
            if k == "lcr" and not (j > 0 and kinds[j - 1] == "seq" and (last_has_nl or j < len(lines) - 1)):
                return "host"                             # a lone CR that is not behind sequence bytes
            if k == ">":
                if seen and length == 0:
                    return "host"
                seen, length = True, 0
            elif not seen and k != "blank":
                return "host"
            elif k == "seq":
                length += klen(c)
        return "host" if seen and length == 0 else "device"
    full = [(c, k) for c, k in zip(lines, kinds) if k not in ("blank", "lcr")]
    if len(full) % 4:
        return "host"                                     # a truncated last record
    o = 0
    for c, k in zip(lines, kinds):
        if k == "lcr" and o % 4:
            return "host"                                 # a lone CR inside a record
        if k not in ("blank", "lcr"):
            if (o % 4 == 0 and k != "@") or (o % 4 == 1 and k != "seq") or (o % 4 == 2 and k != "+"):
                return "host"                             # not four lines: '@', a sequence line, '+', qualities
            o += 1
    for i in range(0, len(full), 4):
        if klen(full[i + 1][0]) != klen(full[i + 3][0]) or klen(full[i + 1][0]) == 0:
            return "host"
    return "device"


# ---------------------------------------------------------------------------------------------------------------- a seeded corpus

SEED, N_TEXTS = 20261021, 300

_NAMES = (b"r", b"ab", b"a/1", b"/1", b"ab/2", b"x/1/2", b"q/12", b"", b"n.7/a", b"longer_name:1:2")
_COMMENTS = (b"", b"", b"", b" ", b" c", b"\tx  y", b" BC:Z:AC\tq", b"\vv", b" \r")
_QFIRST = (b"@", b"+", b">")


def _seq_line(g, n):
    return bytes(g.pick(b"ACGTACGTACGTacgtNRY") for _ in range(n))


def _odd_line(g, eol, odd):
    """the optional lines: blank, CR LF, lone CR"""
    if not g.chance(odd):
        return b""
    return g.pick((b"\n", b"\n", eol, b"\r\n", b"\r\n"))


def random_text(g: _Lcg) -> bytes:
    is_fq = g.chance(500)
    eol = b"\r\n" if g.chance(250) else b"\n"
    odd = 200 if g.chance(550) else 0                      # most texts are regular; some have the optional lines anywhere
    out = []
    if g.chance(60):
        out.append(g.pick((b"\n", b"\n\n", b"\r\n", b"text\n")))
    for _ in range(1 + g.next(6)):
        hdr = (b"@" if is_fq else b">") + g.pick(_NAMES) + g.pick(_COMMENTS) + eol
        out.append(hdr)
        out.append(_odd_line(g, eol, odd // 3))
        if not is_fq:
            for _ in range(1 + g.next(3)):
                out.append(_seq_line(g, 1 + g.next(12)) + eol)
                out.append(_odd_line(g, eol, odd))
            continue
        n = 1 + g.next(12)
        seq = _seq_line(g, n)
        qual = bytes(33 + g.next(41) for _ in range(n)).replace(b"@", b"A")
        if g.chance(200):
            qual = g.pick(_QFIRST) + qual[1:]
        if g.chance(25):
            qual = qual + b"I" if g.chance(500) else qual[:-1]          # a refusal (or, for one base, an empty quality line)
        cut = 1 + g.next(n) if n > 1 and g.chance(40) else n           # a multi-line record
        out.append(seq[:cut] + eol + (seq[cut:] + eol if cut < n else b""))
        out.append(_odd_line(g, eol, odd // 3))
        out.append(b"+" + (g.pick(_NAMES) if g.chance(300) else b"") + eol)
        out.append(_odd_line(g, eol, odd // 3))
        out.append(qual[:cut] + eol + (qual[cut:] + eol if cut < n else b""))
        out.append(_odd_line(g, eol, odd))
    text = b"".join(out)
    if g.chance(250):
        text = text[:-1] if g.chance(700) or not text.endswith(b"\r\n") else text[:-2]           # the last line without its '\n' (and so ending in CR), or without its CR LF
    return text


def random_texts(seed: int = SEED, n: int = N_TEXTS) -> list:
    g = _Lcg(seed)
    return [random_text(g) for _ in range(n)]
