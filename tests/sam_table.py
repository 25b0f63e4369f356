"""The hand-made record tables of test_sam_core.py and test_sam_core_gpu.py: reads with their 16-int records and alignments, the SAM lines they must give
written out literally, and the arrays the writers take (csrc/sam_core.h through tests/sam_core_host.cpp, bmh_format_sam*, the device kernels)."""
import re

import numpy as np

CONTIGS = [("c1", 1000), ("c2", 2000), ("c3_alt", 500)]
_OFF = {"c1": 0, "c2": 1000, "c3_alt": 3000}
S10, T10 = "ACGTACGTAC", "AACCGGTTAC"            # revcomp: GTACGTACGT, GTAACCGGTT


def rec(score, aln=None, mapq=60, flag=0, sub=0, sec=-1, rep=1, alt=0, alt_sc=0, xa=False):
    """a record: aln = (contig, 1-based position, reverse, CIGAR, NM, MD) or None; sec: the record it is listed under ([11] and [12]); xa: an unreported hit
    the XA tag lists (so it needs an alignment unless flag_all)"""
    return dict(score=score, aln=aln, mapq=mapq, flag=flag, sub=sub, sec=sec, rep=rep, alt=alt, alt_sc=alt_sc, xa=xa)


def hits(scores, n_aln, last_alt=False):
    """unreported hits under record 0, the k-th at c2:100k+1 on alternating strands with NM k; only the first n_aln carry an alignment"""
    out = []
    for k, sc in enumerate(scores, 1):
        a = ("c2", 100 * k + 1, int(k % 2 == 0), "10M", k, "10")
        if last_alt and k == len(scores):
            a = ("c3_alt", 51, 1, "10M", k, "10")
        out.append(rec(sc, aln=a if k <= n_aln else None, mapq=0, sec=0, rep=0, alt=int(last_alt and k == len(scores)), xa=k <= n_aln))
    return out


def read(name, seq, recs, qual=None, comment="", h=-1, unflag=0):
    return dict(name=name, seq=seq, recs=recs, qual=qual or "I" * len(seq), comment=comment, h=h, unflag=unflag)


SE = [
    read("fwd", "ACGTRACGTA", [rec(10, ("c1", 100, 0, "10M", 0, "10"))], "ABCDEFGHIJ", "BC:Z:x1"),                       # a base that is not ACGT
    read("rev", T10, [rec(7, ("c2", 5, 1, "2S8M", 1, "3A4"), mapq=30, sub=3)], "0123456789", ""),
    read("split", S10, [rec(6, ("c1", 201, 0, "6M4S", 0, "6")), rec(4, ("c2", 301, 1, "6S4M", 0, "4"), mapq=20, flag=0x800),
                        rec(4, ("c1", 501, 0, "3S4M3S", 0, "4"), mapq=10, flag=0x800)], "abcdefghij", "XY:i:7"),
    read("sec", S10, [rec(10, ("c1", 11, 0, "10M", 0, "10"), mapq=0, sub=9), rec(9, ("c2", 11, 0, "10M", 1, "5C4"), mapq=0, flag=0x100, sec=0)]),
    # five listed hits and one at exactly 80 % of the primary's score, which is out (counted, it would make six and silence the tag)
    read("xa5", S10, [rec(50, ("c1", 301, 0, "10M", 0, "10"), mapq=0, sub=45)] + hits([45, 44, 43, 42, 41, 40], 5)),
    read("xa6", S10, [rec(50, ("c1", 401, 0, "10M", 0, "10"), mapq=0, sub=46)] + hits([46, 45, 44, 43, 42, 41], 0)),
    read("xaalt", S10, [rec(50, ("c1", 601, 0, "10M", 0, "10"), mapq=0, sub=46)] + hits([46, 45, 44, 43, 42, 41], 6, last_alt=True)),
    read("paf", S10, [rec(1, ("c1", 701, 0, "10M", 0, "10"), mapq=0, alt_sc=16)]),
    read("unm", S10, [rec(5, rep=0)]),
    read("none", S10, [], "KLMNOPQRST", "co:Z:none"),
]
_TAIL = "\t*\tNM:i:0\tMD:Z:10\tAS:i:"
_XA5 = "c2,+101,10M,1;c2,-201,10M,2;c2,+301,10M,3;c2,-401,10M,4;c2,+501,10M,5;"
SE_LINES = [
    "fwd\t0\tc1\t100\t60\t10M\t*\t0\t0\tACGTNACGTA\t*\tNM:i:0\tMD:Z:10\tAS:i:10\tXS:i:0",
    "rev\t16\tc2\t5\t30\t2S8M\t*\t0\t0\tGTAACCGGTT\t*\tNM:i:1\tMD:Z:3A4\tAS:i:7\tXS:i:3",
    "split\t0\tc1\t201\t60\t6M4S\t*\t0\t0\tACGTACGTAC\t*\tNM:i:0\tMD:Z:6\tAS:i:6\tXS:i:0\tSA:Z:c2,301,-,6S4M,20,0;c1,501,+,3S4M3S,10,0;",
    "split\t2064\tc2\t301\t20\t6H4M\t*\t0\t0\tACGT\t*\tNM:i:0\tMD:Z:4\tAS:i:4\tXS:i:0\tSA:Z:c1,201,+,6M4S,60,0;c1,501,+,3S4M3S,10,0;",
    "split\t2048\tc1\t501\t10\t3H4M3H\t*\t0\t0\tTACG\t*\tNM:i:0\tMD:Z:4\tAS:i:4\tXS:i:0\tSA:Z:c1,201,+,6M4S,60,0;c2,301,-,6S4M,20,0;",
    "sec\t0\tc1\t11\t0\t10M\t*\t0\t0\tACGTACGTAC\t*\tNM:i:0\tMD:Z:10\tAS:i:10\tXS:i:9\tXA:Z:c2,+11,10M,1;",
    "sec\t256\tc2\t11\t0\t10M\t*\t0\t0\t*\t*\tNM:i:1\tMD:Z:5C4\tAS:i:9",
    "xa5\t0\tc1\t301\t0\t10M\t*\t0\t0\tACGTACGTAC" + _TAIL + "50\tXS:i:45\tXA:Z:" + _XA5,
    "xa6\t0\tc1\t401\t0\t10M\t*\t0\t0\tACGTACGTAC" + _TAIL + "50\tXS:i:46",
    "xaalt\t0\tc1\t601\t0\t10M\t*\t0\t0\tACGTACGTAC" + _TAIL + "50\tXS:i:46\tXA:Z:" + _XA5 + "c3_alt,-51,10M,6;",
    "paf\t0\tc1\t701\t0\t10M\t*\t0\t0\tACGTACGTAC" + _TAIL + "1\tXS:i:0\tpa:f:0.062",
    "unm\t4\t*\t0\t0\t*\t*\t0\t0\tACGTACGTAC\t*\tAS:i:0\tXS:i:0",
    "none\t4\t*\t0\t0\t*\t*\t0\t0\tACGTACGTAC\t*\tAS:i:0\tXS:i:0",
]
# -Y: soft clips and the whole read on the later records too
SOFT = [SE[2]]
SOFT_LINES = [
    SE_LINES[2],
    "split\t2064\tc2\t301\t20\t6S4M\t*\t0\t0\tGTACGTACGT\t*\tNM:i:0\tMD:Z:4\tAS:i:4\tXS:i:0\tSA:Z:c1,201,+,6M4S,60,0;c1,501,+,3S4M3S,10,0;",
    "split\t2048\tc1\t501\t10\t3S4M3S\t*\t0\t0\tACGTACGTAC\t*\tNM:i:0\tMD:Z:4\tAS:i:4\tXS:i:0\tSA:Z:c1,201,+,6M4S,60,0;c2,301,-,6S4M,20,0;",
]
# -a: no XA tag, and the hits it would have listed need no alignment
ALL = [SE[3], SE[4], SE[6]]
ALL_LINES = [
    "sec\t0\tc1\t11\t0\t10M\t*\t0\t0\tACGTACGTAC\t*\tNM:i:0\tMD:Z:10\tAS:i:10\tXS:i:9",
    SE_LINES[6],
    "xa5\t0\tc1\t301\t0\t10M\t*\t0\t0\tACGTACGTAC" + _TAIL + "50\tXS:i:45",
    "xaalt\t0\tc1\t601\t0\t10M\t*\t0\t0\tACGTACGTAC" + _TAIL + "50\tXS:i:46",
]
# -R, -C and the qualities of a FASTQ file: RG behind AS / XS and in front of SA, the comment last (an empty one is not written), QUAL reversed on the reverse strand
TAGS = [SE[0], SE[1], SE[2], SE[9]]
TAGS_LINES = [
    "fwd\t0\tc1\t100\t60\t10M\t*\t0\t0\tACGTNACGTA\tABCDEFGHIJ\tNM:i:0\tMD:Z:10\tAS:i:10\tXS:i:0\tRG:Z:grp1\tBC:Z:x1",
    "rev\t16\tc2\t5\t30\t2S8M\t*\t0\t0\tGTAACCGGTT\t9876543210\tNM:i:1\tMD:Z:3A4\tAS:i:7\tXS:i:3\tRG:Z:grp1",
    "split\t0\tc1\t201\t60\t6M4S\t*\t0\t0\tACGTACGTAC\tabcdefghij\tNM:i:0\tMD:Z:6\tAS:i:6\tXS:i:0\tRG:Z:grp1\tSA:Z:c2,301,-,6S4M,20,0;c1,501,+,3S4M3S,10,0;\tXY:i:7",
    "split\t2064\tc2\t301\t20\t6H4M\t*\t0\t0\tACGT\tdcba\tNM:i:0\tMD:Z:4\tAS:i:4\tXS:i:0\tRG:Z:grp1\tSA:Z:c1,201,+,6M4S,60,0;c1,501,+,3S4M3S,10,0;\tXY:i:7",
    "split\t2048\tc1\t501\t10\t3H4M3H\t*\t0\t0\tTACG\tdefg\tNM:i:0\tMD:Z:4\tAS:i:4\tXS:i:0\tRG:Z:grp1\tSA:Z:c1,201,+,6M4S,60,0;c2,301,-,6S4M,20,0;\tXY:i:7",
    "none\t4\t*\t0\t0\t*\t*\t0\t0\tACGTACGTAC\tKLMNOPQRST\tAS:i:0\tXS:i:0\tRG:Z:grp1\tco:Z:none",
]


def _pair(name, a, b):
    """a, b: (record or None, flags of mem_sam_pe in [14] / of the unmapped record)"""
    return [read(name, s, [x[0]] if x[0] else [], h=0 if x[0] else -1, unflag=x[1]) for s, x in ((S10, a), (T10, b))]


_M = lambda ctg, pos, rev, flag: (rec(10, (ctg, pos, rev, "10M", 0, "10"), flag=flag), flag)
PE = (_pair("pA", _M("c1", 101, 0, 0x43), _M("c1", 151, 1, 0x83)) +        # same contig: TLEN 60 and -60
      _pair("pB", _M("c1", 201, 0, 0x41), _M("c1", 201, 0, 0x81)) +        # the same leftmost base: TLEN 0
      _pair("pC", _M("c1", 301, 0, 0x41), _M("c2", 401, 1, 0x81)) +        # different contigs
      _pair("pD", _M("c2", 501, 1, 0x41), (None, 0x81)) +                  # one mate unmapped: each lends the other its coordinate and strand
      _pair("pF", (None, 0x41), _M("c1", 801, 0, 0x81)) +
      _pair("pE", (None, 0x41), (None, 0x81)))                             # both unmapped
_PT = "\t*\tNM:i:0\tMD:Z:10\tAS:i:10\tXS:i:0"
PE_LINES = [
    "pA\t99\tc1\t101\t60\t10M\t=\t151\t60\tACGTACGTAC" + _PT,
    "pA\t147\tc1\t151\t60\t10M\t=\t101\t-60\tGTAACCGGTT" + _PT,
    "pB\t65\tc1\t201\t60\t10M\t=\t201\t0\tACGTACGTAC" + _PT,
    "pB\t129\tc1\t201\t60\t10M\t=\t201\t0\tAACCGGTTAC" + _PT,
    "pC\t97\tc1\t301\t60\t10M\tc2\t401\t0\tACGTACGTAC" + _PT,
    "pC\t145\tc2\t401\t60\t10M\tc1\t301\t0\tGTAACCGGTT" + _PT,
    "pD\t121\tc2\t501\t60\t10M\t=\t501\t0\tGTACGTACGT" + _PT,
    "pD\t181\tc2\t501\t0\t*\t=\t501\t0\tGTAACCGGTT\t*\tAS:i:0\tXS:i:0",
    "pF\t69\tc1\t801\t0\t*\t=\t801\t0\tACGTACGTAC\t*\tAS:i:0\tXS:i:0",
    "pF\t137\tc1\t801\t60\t10M\t=\t801\t0\tAACCGGTTAC" + _PT,
    "pE\t77\t*\t0\t0\t*\t*\t0\t0\tACGTACGTAC\t*\tAS:i:0\tXS:i:0",
    "pE\t141\t*\t0\t0\t*\t*\t0\t0\tAACCGGTTAC\t*\tAS:i:0\tXS:i:0",
]
# (reads, lines, options, paired)
CASES = {
    "default": (SE, SE_LINES, {}, False), "softclip": (SOFT, SOFT_LINES, dict(softclip=1), False), "flag_all": (ALL, ALL_LINES, dict(flag_all=1), False),
    "rg_comment_qual": (TAGS, TAGS_LINES, dict(rg_id=b"grp1", copy_comment=1), False), "pairs": (PE, PE_LINES, {}, True),
}


class Table:
    """the arrays of a list of reads.  need: the selection the table implies -- reported, an XA hit (not with flag_all), a read's own alignment (pairs)"""

    def __init__(self, reads, flag_all=False, paired=False, contigs=CONTIGS):
        off = dict(zip([c[0] for c in contigs], np.concatenate([[0], np.cumsum([c[1] for c in contigs])[:-1]])))
        self.contigs, self.paired, self.n = contigs, paired, len(reads)
        self.names = [r["name"] for r in reads]
        self.comments = [r["comment"] for r in reads]
        self.lens = np.array([len(r["seq"]) for r in reads], np.uint32)
        self.offs = np.concatenate([[0], np.cumsum(self.lens)[:-1]]).astype(np.uint64)
        self.ascii = np.frombuffer("".join(r["seq"] for r in reads).encode(), np.uint8).copy()
        self.quals = np.frombuffer("".join(r["qual"] for r in reads).encode(), np.uint8).copy()
        self.codes = np.full(256, 4, np.uint8)
        for k, c in enumerate("ACGT"):
            self.codes[ord(c)] = self.codes[ord(c.lower())] = k
        self.codes = self.codes[self.ascii]
        self.fpr = np.array([len(r["recs"]) for r in reads], np.uint32)
        self.h_rec = np.array([r["h"] for r in reads], np.int32)
        self.unflag = np.array([r["unflag"] for r in reads], np.int32)
        fin, need, alns = [], [], []
        for i, r in enumerate(reads):
            for j, x in enumerate(r["recs"]):
                f = [0] * 16
                f[0], f[1], f[10], f[11], f[12], f[13], f[14], f[15] = i, x["score"], x["sub"], x["sec"], x["sec"], x["mapq"], x["flag"], x["rep"] | x["alt"] << 1 | x["alt_sc"] << 2
                fin.append(f)
                need.append(int(bool(x["rep"] or (x["xa"] and not flag_all) or (paired and j == r["h"]))))
                if need[-1]:
                    alns.append(x["aln"])
        self.fin = np.array(fin, np.int32).reshape(-1, 16)
        self.need = np.array(need, np.uint8)
        self.slot = np.where(self.need, np.cumsum(self.need) - 1, -1).astype(np.int64)
        k = len(alns)
        ops = [[(int(n), "MIDSH".index(c)) for n, c in re.findall(r"(\d+)([MIDSH])", a[3])] for a in alns]
        self.cigar = np.zeros((max(k, 1), max([len(o) for o in ops] + [4])), np.uint32)
        self.md = np.zeros((max(k, 1), 8), np.uint8)
        self.aln = np.zeros((max(k, 1), 8), np.int32)
        for s, (a, o) in enumerate(zip(alns, ops)):
            pos = int(off[a[0]]) + a[1] - 1
            self.aln[s] = [pos & 0xFFFFFFFF, pos >> 32, a[2], len(o), a[4], 0, len(a[5]), 0]
            self.cigar[s, :len(o)] = [n << 4 | c for n, c in o]
            self.md[s, :len(a[5])] = np.frombuffer(a[5].encode(), np.uint8)
        self.aln, self.cigar, self.md = self.aln[:k], self.cigar[:k], self.md[:k]
        # the packed form of bmh_cigar_pack: the operations, then the MD string with its NUL padded to a word
        words = [np.concatenate([self.cigar[s, :self.aln[s, 3]], self.md[s, :(self.aln[s, 6] + 4) // 4 * 4].view(np.uint32)]) for s in range(k)]
        self.cig_off = np.concatenate([[0], np.cumsum([len(w) for w in words])]).astype(np.uint32)
        self.packed = np.concatenate(words + [np.zeros(1, np.uint32)]).astype(np.uint32)

    def blob(self, strings, dt=np.uint64):
        enc = [s.encode() + b"\0" for s in strings]
        return np.frombuffer(b"".join(enc) or b"\0", np.uint8).copy(), np.concatenate([[0], np.cumsum([len(e) for e in enc])]).astype(dt)

    def write(self, path, opts, with_quals):
        """the table file of tests/sam_core_host.cpp"""
        o = np.array([opts.get("flag_all", 0), opts.get("softclip", 0), 12, 5, 200, int(self.paired), opts.get("copy_comment", 0), len(self.contigs)], np.int32)
        nb, no = self.blob(self.names)
        cb, co = self.blob(self.comments)
        gb, go = self.blob([c[0] for c in self.contigs], np.uint32)
        coff = np.concatenate([[0], np.cumsum([c[1] for c in self.contigs])[:-1]]).astype(np.int64)
        secs = [o, np.array([float(np.float32(0.8))]), np.frombuffer(opts.get("rg_id", b""), np.uint8), self.fpr, self.fin, self.slot.astype(np.int32), self.aln, self.cig_off,
                self.packed, nb, no, self.ascii, self.offs, self.lens, self.quals if with_quals else np.zeros(0, np.uint8), cb, co, gb, go, coff, self.h_rec, self.unflag]
        with open(path, "wb") as f:
            for a in secs:
                b = np.ascontiguousarray(a).tobytes()
                f.write(np.int64(len(b)).tobytes() + b + b"\0" * (-len(b) % 8))

    def host_text(self, po, with_quals=False, with_comments=False) -> bytes:
        """bmh_format_sam[_pe][_ex] on the table with the fixed CIGAR slots"""
        from bwamem_hip.lib import format_sam
        nb, no = self.blob(self.names)
        cb, co = self.blob(self.comments)
        return format_sam(po, (nb, no[:-1]), self.codes, self.offs, self.lens, self.contigs, self.fin, self.fpr, self.slot, self.aln.reshape(-1, 8),
                          self.cigar, self.md, h_rec=self.h_rec if self.paired else None, unflag=self.unflag if self.paired else None, as_bytes=True,
                          quals=self.quals if with_quals else None, comments=(cb, co[:-1]) if with_comments else None)


def post_opt(opts):
    import ctypes as C
    from bwamem_hip.lib import PostOpt, load_library
    po = PostOpt(); load_library().bmh_post_opt_default(C.byref(po))
    for k, v in opts.items():
        setattr(po, k, v)
    return po
