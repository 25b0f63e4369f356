// Internal declarations shared by the translation units of libbwamem_hip.so.
#pragma once
#include "../../include/bwamem_hip.h"
#include "fmd_dev.h"

struct bmh_index {
	fmd_dev_t dev;
	bool owns;             // arrays were hipMalloc'd by bmh_index_upload
	bool owns_sa;          // sa / sa_bits were replaced by bmh_index_densify_sa (its own allocations)
	bool owns_blocks;      // dev.blocks is the handle's own native re-encoding of a caller's buffer (bmh_index_from_device)
	uint64_t n_words;
};
// csrc/kmer_bits.hip: the handle's K-mer bitmap (dev.kbits), built on the current device -- every function that gives a handle a text
// calls attach once the text is in place (a handle copied from another must not keep the other's pointer); free with the handle
void bmh_kbits_attach(bmh_index *ix);
void bmh_kbits_free(bmh_index *ix);

// extension jobs described by where their bases live instead of materialised base arrays (device job builder)
struct bmh_ext_desc_t {
	const uint8_t *reads;        // ASCII reads of the batch
	const uint8_t *pac; long long l_pac;     // 2-bit forward strand
	const uint32_t *jq_src;      // [n] offset of the query segment in reads
	const uint32_t *job_side;    // [n] 0 = LEFT (both sequences run backwards), 1 = RIGHT
	uint32_t max_qlen;           // 0, or an upper bound of every query length of the batch (the longest read): classes no job can reach are not launched
	const int64_t *jt0;          // [n] first text position of the target window; a window lies on ONE strand of fwd . revcomp(fwd)
	                             // (mem_chain2aln clips it at l_pac, src/bwamem.c:1261-1264): the kernels decode eight rows at a time on that premise
	uint32_t long_cap;           // 0, or the cap of bmh_extend_batch_long: query sides of 769 .. long_cap bases run on the long-query classes
};
int bmh_extend_batch_desc(const bmh_ext_desc_t *desc, const uint32_t *d_qlen, const uint32_t *d_tlen, const uint32_t *d_h0, uint32_t n,
                          const bmh_ext_params_t *p, int32_t *d_out, int32_t *d_raw, void *stream);
// sizes the extension's per-(device, stream) scratch for batches of up to n jobs (a later growth frees device memory, which waits for the device)
int bmh_extend_reserve(void *stream, uint64_t n);

#ifdef __cplusplus
#include <functional>
#include <string>
#include <vector>
// where the formatter finds a record's alignment: slot (64- or 32-bit, -1 = none) -> aln[8], and the operations / MD string either in the
// fixed slots bmh_cigar_batch writes or in the packed words of bmh_cigar_pack (off[s] = first word of alignment s: its operations, then
// its MD string)
struct bmh_cigar_src_t {
	const int64_t *slot64 = nullptr; const int32_t *slot32 = nullptr;
	const int32_t *aln = nullptr;
	const uint32_t *cigar = nullptr; int max_cigar = 0; const char *md = nullptr; int md_cap = 0;
	const uint32_t *packed = nullptr; const uint32_t *off = nullptr; bool packed_md = true;
};
// bmh_format_sam / bmh_format_sam_pe (h_rec, unflag: the pairs' arrays, NULL for single-end reads) as the parts the formatting threads
// made, in order; `parts` is reused by the caller (csrc/sam_format.cpp, csrc/align_pipeline.hip)
bool bmh_format_sam_parts(const bmh_post_opt_t *po, uint32_t n_reads, const char *names, const uint64_t *name_off, const uint8_t *reads,
                          const uint64_t *read_offs, const uint32_t *read_lens, int n_contigs, const char *const *contig_names,
                          const int64_t *contig_offset, const int32_t *fin, const uint32_t *fin_per_read, const bmh_cigar_src_t &cs,
                          const int32_t *h_rec, const int32_t *unflag, std::vector<std::string> &parts,
                          const uint8_t *quals = nullptr, const char *comments = nullptr, const uint64_t *comment_off = nullptr,
                          const bmh_read_groups_t *groups = nullptr);       // groups: a read group per read (include/bwamem_hip.h), checked by the caller
// csrc/sam_kernels.hip, for csrc/align_pipeline.hip: the alignments whose fixed slots overflowed (flags 1, 8) found and, once redone with large
// slots, put in place on the device (see the definitions)
int64_t bmh_cigar_overflowed(const int32_t *d_aln, uint32_t n, const uint32_t *d_sel, uint32_t *d_over, uint32_t *d_sel2, uint32_t *d_counter, void *stream);
size_t bmh_cigar_patch_work(uint32_t n_over);
int64_t bmh_cigar_patch(int32_t *d_aln, uint32_t *d_off, uint32_t *d_packed, uint64_t words, const uint32_t *d_over, uint32_t n_over,
                        const int32_t *d_aln2, const uint32_t *d_cigar2, int mc2, const char *d_md2, int mdc2, void *d_work, size_t work_bytes, void *stream);
// csrc/regs_kernels.hip: bmh_finalize_regs_device with by-products (in: d_dedup_out [n_regs][16] or NULL, d_out_off [n_reads] or NULL; out: the device's
// logarithm table and contig offsets, valid until the stream's scratch is released; alt_keep_sub_n: with an ALT table [11] stays sub_n -- regs_core.h ctx_t)
struct bmh_fin_extra_t { int32_t *d_dedup_out; uint32_t *d_out_off; const double *d_logtab; int n_log; const int64_t *d_ctg_off; int alt_keep_sub_n; };
int64_t bmh_finalize_regs_device_ex(const bmh_index_t *idx, const bmh_chain_opt_t *copt, const bmh_ext_params_t *ep, const bmh_post_opt_t *popt,
                                    const uint8_t *d_reads, const uint32_t *d_offs, uint32_t n_reads,
                                    const int32_t *d_regs, uint64_t n_regs, const uint32_t *d_regs_per_read, const float *d_frac_rep,
                                    int n_contigs, const int64_t *contig_offset, int32_t *d_out, uint32_t *d_out_per_read, void *stream, bmh_fin_extra_t *extra);
// csrc/sam_kernels.hip: the device tail's records as ALT-mode records ([11] = [12]), then the records of the ns reads the host redid with the ALT table (d_ids, their
// records d_sub at d_sub_off [ns + 1]) in their places (d_rec_off: first record of every read)
int bmh_alt_records_device(int32_t *d_fin, uint64_t m, const uint32_t *d_rec_off, const uint32_t *d_ids, const uint32_t *d_sub_off, const int32_t *d_sub, uint32_t ns, void *stream);
// csrc/reads_io.cpp: a mapped read file cut and filled batch by batch (bmh_aligner_run_fasta, bmh_aligner_run_file).  fmt.fq: FASTQ records (4 lines;
// a record starts at a '@' line whose line two below starts with '+'), else FASTA; fmt.comments: count (cut) and fill the header comments too -- the fill
// writes o->quals (FASTQ) and o->comments / o->comment_offs when they are not NULL; fmt.either: the caller takes either layout (its messages name the FASTQ
// problems; a FASTA-only caller keeps its one message).  bmh_reads_detect: 1 when the first non-blank byte is '@'
struct bmh_reads_fmt_t { bool fq = false; bool comments = false; bool either = false; };
int bmh_reads_detect(const uint8_t *buf, size_t sz);
int bmh_map_file(const char *fn, const char *path, const uint8_t **buf, size_t *sz);        // the file mapped for reading (the caller's to munmap); *sz = 0: empty, nothing mapped
int bmh_fasta_cut(const uint8_t *buf, size_t sz, size_t p, uint64_t want_bases, uint64_t want_reads, bool even, int n_threads, size_t est_bytes,
                  size_t *end, uint64_t *n_reads, uint64_t *n_bases, uint64_t *n_name_bytes, const bmh_reads_fmt_t &fmt = bmh_reads_fmt_t(),
                  uint64_t *n_comment_bytes = nullptr);
int bmh_fasta_fill(const uint8_t *buf, size_t p, size_t end, uint64_t n_reads, uint64_t n_bases, uint64_t n_name_bytes, int n_threads, bmh_read_set_t *o,
                   const bmh_reads_fmt_t &fmt = bmh_reads_fmt_t(), uint64_t n_comment_bytes = 0);
// ---- read files of any shape (bmh_reads_load_files, bmh_aligner_run_files): multi-line records, gzip / BGZF, two files
// csrc/reads_src.cpp: the text of a plain, gzip or BGZF file (or pipe) in order; n_threads: host threads of the BGZF inflate (<= 0: bmh_effective_cpus)
struct bmh_text_src_t;
bmh_text_src_t *bmh_text_open(const char *path, int n_threads);          // NULL: the message is set
int64_t bmh_text_read(bmh_text_src_t *s, uint8_t *dst, size_t n);         // bytes written: fewer than n at the end of the text only; -1: error (message set)
int bmh_text_kind(const bmh_text_src_t *s);                              // 0 plain, 1 gzip, 2 BGZF
void bmh_text_close(bmh_text_src_t *s);
// a BGZF source for the device inflate (csrc/inflate_kernels.hip): whole compressed members into dst [cap >= bmh_text_pending + 1 MiB] until they hold want_text bytes of
// text, the file ends or dst is full; tab: one entry per member (offsets into dst / into their text); returns the bytes they cover, -1: refused; *end: nothing is left
size_t bmh_text_pending(const bmh_text_src_t *s);
int64_t bmh_text_members(bmh_text_src_t *s, uint8_t *dst, size_t cap, size_t want_text, std::vector<bmh_inflate_member_t> &tab, uint64_t *text_bytes, bool *end);
uint64_t bmh_text_host_members(const bmh_text_src_t *s);                // BGZF members inflated by the host threads so far
// csrc/reads_io.cpp: the host walker (kseq_read restated) appends a record to growing arrays; nlen / clen: bytes of its name / comment with their NUL
struct bmh_hbatch_t {
	std::vector<uint8_t> ascii, quals, names, comments; std::vector<uint32_t> lens, nlen, clen, grp;      // grp: a BAM run that keeps read groups -- every read's
	void clear() { ascii.clear(); quals.clear(); names.clear(); comments.clear(); lens.clear(); nlen.clear(); clen.clear(); grp.clear(); }
};
int bmh_walk_record(const uint8_t *b, size_t n, bool eof, size_t *p, bmh_hbatch_t &o, bool comments, int *kind);
void bmh_nt4_codes(const uint8_t *src, uint8_t *dst, size_t n);
// csrc/reads_parse.hip: one or two read files batch by batch -- text windows in (pinned) host memory, cut into records by the device parser or, for what it
// hands back (and with host_only), by the host walker.  next: 1 = a batch in the arrays `alloc` provided (it is told the sizes and sets rs's pointers; offsets
// start at 0), 0 = the end, < 0 = refused.  The batch ends as bseq_read ends its batches (bases >= want_bases -- or reads == want_reads if not 0 -- and an
// even count when `even`; pairs stay together with two files); take_all: every complete record of the window instead.
struct bmh_reads_pump_t;
struct bmh_rg_table_t;
typedef std::function<int(uint64_t n_reads, uint64_t n_bases, uint64_t n_name_bytes, uint64_t n_comment_bytes, bool fq, bmh_read_set_t *rs)> bmh_batch_alloc_t;
// keep_rg / markdup: the input must be one BAM, its header's @RG lines become the run's read groups (bmh_pump_read_groups) and every read carries its own (rs->groups)
// collate: a BAM's mates are collated by name (csrc/bam_collate_core.h), collate_mem: the cap on its open records' bytes (0: 8 GiB); text input ignores both -- the
// caller that must refuse it asks bmh_pump_bam_paired
bmh_reads_pump_t *bmh_pump_open(const char *path1, const char *path2, int n_threads, bool comments, bool host_only, size_t chunk_bytes, bool keep_rg = false, bool markdup = false,
                                bool collate = false, uint64_t collate_mem = 0);
void bmh_pump_collate_counts(const bmh_reads_pump_t *p, uint64_t out[5]);   // of a pump that collates, else zeros
bool bmh_pump_collate_ended_open(const bmh_reads_pump_t *p);                // its refusal was that of a record still open at the file's end
const bmh_rg_table_t *bmh_pump_read_groups(const bmh_reads_pump_t *p);   // of a pump opened with keep_rg, else NULL
int bmh_pump_next(bmh_reads_pump_t *p, uint64_t want_bases, uint64_t want_reads, bool even, bool take_all, const bmh_batch_alloc_t &alloc, bmh_read_set_t *rs);
void bmh_pump_counts(const bmh_reads_pump_t *p, uint64_t out[4]);        // windows parsed on the device, windows walked on the host, text bytes, records
void bmh_pump_close(bmh_reads_pump_t *p);
// for the tests and scripts/reads_input_rate.py, not part of the public interface: out[4] of the process's last bmh_reads_load_files / bmh_aligner_run_files call --
// windows cut on the device, windows walked by the host, text bytes, records
void bmh_reads_note_counts(const uint64_t *c);
extern "C" int bmh_reads_last_counts(uint64_t *out);
// beside it: out[2] of the same call -- BGZF members inflated on the device, BGZF members inflated by the host threads
void bmh_pump_inflate_counts(const bmh_reads_pump_t *p, uint64_t out[2]);
void bmh_reads_note_inflate_counts(const uint64_t *c);
extern "C" int bmh_reads_last_inflate_counts(uint64_t *out);
// ---- BAM as read input (csrc/bam_in_core.h): a BGZF file whose text begins with "BAM\1" is the pump's third kind.  A BAM record names its own length, so the
// record starts of a window are one dependent chain: the host walks it over the window it has just inflated (bmh_bam_chain: one 4-byte read per record); BAM
// therefore always takes the host inflate.  Everything else is done per record, base and read on the device (csrc/bam_in_kernels.hip: bmh_bam_dev_run) or, as
// the definition, the fallback that words the refusals and the form without a device, on the host (csrc/reads_io.cpp: bmh_bam_host_run).
// csrc/reads_src.cpp: 0 text, 1 a BGZF file that holds a BAM, 2 a plain gzip stream that holds one (refused); looked at without taking a byte of the text
int bmh_text_bam(bmh_text_src_t *s);
// the whole BAM header (magic, text, reference table) at the front of b[0, n): its bytes, 0 when it is not whole yet, -1 when the bytes are no BAM header
int64_t bmh_bam_header_bytes(const uint8_t *b, size_t n);
// the record starts of b[0, n) -> starts (one more entry: the end of the last whole record); a record is whole when start + 4 + block_size <= n
void bmh_bam_chain(const uint8_t *b, size_t n, std::vector<uint32_t> &starts);
// the same walk taken up where it stood: starts is not empty, its last entry is the end of the last whole record found so far (0 at first)
void bmh_bam_chain_extend(const uint8_t *b, size_t n, std::vector<uint32_t> &starts);
extern "C" int bmh_bam_chain_count(const uint8_t *records, uint64_t n_bytes, uint64_t *n_records, uint64_t *end);   // the walk alone, timed by scripts/reads_input_rate.py --bam-only
// the flag of the first record of b[0, n) that gives a read: 1 and *flag, or 0 when the whole records of b hold none (yet)
int bmh_bam_first_kept(const uint8_t *b, size_t n, uint32_t *flag);      // (-1: a record too short for its fixed fields comes first)
// what a BAM file's windows share.  paired: flag 0x1 of the first record kept; qual: 0 unknown, 1 the records have qualities, 2 they have none
// rg_ids / rg_off: a run that keeps the input's read groups -- the IDs of the header's @RG lines back to back with offsets [n + 1] (bi_groups_t); empty: no tag is read.
// Such a run writes every read's group index to rs->groups when the allocator has provided the array.
// col: mates are collated by name (--collate; csrc/bam_collate_core.h has the definition) -- the pool of open records that both forms work on; NULL: a pair's two
// records are adjacent, as ever.  It changes nothing for a file without flag 0x1.
struct bcl_pool_t;
struct bmh_bam_state_t {
	std::string path; int paired = 0, qual = 0; uint64_t n_recs = 0, n_skipped = 0, n_tags_left_out = 0;
	std::string rg_ids; std::vector<uint32_t> rg_off;
	bcl_pool_t *col = nullptr;
	bool keep_rg() const { return rg_off.size() > 1; }
	bool collate() const { return col != nullptr && paired != 0; }
};
// the pool of a run that collates (mem_bytes 0: the default cap of 8 GiB; the hash width is the knob COLLATE_HASH_BITS), its end, and its counts (out[5]: pairs,
// pairs_adjacent, open_records_peak, open_bytes_peak, windows_to_host_for_hash_runs).  bmh_bam_collate_end: the file has ended and every batch is delivered --
// BMH_OK, or the refusal that names the open record with the smallest index
bcl_pool_t *bmh_bam_collate_create(uint64_t mem_bytes);
void bmh_bam_collate_free(bcl_pool_t *p);
bool bmh_bam_collate_ended_open(const bcl_pool_t *p);                    // the refusal was bmh_bam_collate_end's (or the host form's, of a window's own open record); p may be NULL
int bmh_bam_collate_end(const bmh_bam_state_t &st);
void bmh_bam_collate_counts(const bcl_pool_t *p, uint64_t out[5]);
void bmh_reads_note_collate_counts(const uint64_t *c);
// The @RG lines of a BAM header's text (it ends at its first NUL; the last line may lack its newline; a CR before the newline is dropped; other lines are ignored):
// lines verbatim without their line ends, their IDs, and every group's library index by first appearance (the LB field as bwamem_hip.aligner.rg_library reads it:
// the last non-empty one, groups without one share "Unknown Library") with the libraries' names.  Refused (BMH_EINVAL, the line named, `what` in front): no @RG line, a line
// without a non-empty ID of at most 255 bytes or with a field that is not XX:value, a repeated ID, more than 65535 groups, and with markdup more than 255 libraries.
struct bmh_rg_table_t {
	std::vector<std::string> lines, ids, lib_names; std::vector<int32_t> lib;
	void clear() { lines.clear(); ids.clear(); lib_names.clear(); lib.clear(); }
};
int bmh_bam_header_groups(const char *what, const char *text, size_t n, bool markdup, bmh_rg_table_t &T);
// chain: the record starts of buf[0, have) when the caller has walked them already (bmh_bam_chain's result), else NULL
struct bmh_bam_win_t { const uint8_t *buf; size_t have; bool eof, comments; uint64_t want_bases, want_reads; bool even, take_all; const std::vector<uint32_t> *chain; };
// consumed: the end of the last record taken; n_recs: the records before it; skipped / tags_left_out: among those; qual: the state behind them
struct bmh_bam_res_t { uint64_t n_reads = 0; bool complete = false, final_ = false; size_t consumed = 0; uint64_t n_recs = 0, skipped = 0, tags_left_out = 0; int qual = 0; };
int bmh_bam_host_run(const bmh_bam_state_t &st, const bmh_bam_win_t &w, const bmh_batch_alloc_t &alloc, bmh_read_set_t *rs, bmh_bam_res_t &R, bmh_hbatch_t &hb);   // 1, or < 0: refused
struct bmh_bam_dev_t;
bmh_bam_dev_t *bmh_bam_dev_create();
void bmh_bam_dev_free(bmh_bam_dev_t *d);
int bmh_bam_dev_run(bmh_bam_dev_t *d, const bmh_bam_state_t &st, const bmh_bam_win_t &w, const bmh_batch_alloc_t &alloc, bmh_read_set_t *rs, bmh_bam_res_t &R);   // 1, 2: the window is the host's, < 0
int bmh_bam_reads_run(const char *fn, bmh_bam_dev_t *d, const uint8_t *records, uint64_t n_bytes, int flags, bmh_read_set_t *out, const char *const *rg_ids = nullptr, int n_groups = 0, uint64_t collate_mem = 0);   // csrc/reads_io.cpp: bmh_bam_reads_device / _host
// the pump's answer for bmh_aligner_run_files: -1 the input is no BAM, else flag 0x1 of its first record kept
int bmh_pump_bam_paired(const bmh_reads_pump_t *p);
void bmh_pump_bam_counts(const bmh_reads_pump_t *p, uint64_t out[2]);    // records skipped (0x100 / 0x800), f and B tags left out
void bmh_reads_note_bam_counts(const uint64_t *c);
// the end of the batch among n reads of these lengths (step: 1, or 2 when pairs stay together); *complete: the wanted size was reached -- bseq_read's rule
inline uint64_t bmh_cut_batch(const uint32_t *lens, uint64_t n, int step, uint64_t want_bases, uint64_t want_reads, bool even, bool *complete)
{
	uint64_t acc = 0;
	*complete = false;
	for (uint64_t r = 0; r + step <= n;) {
		for (int k = 0; k < step; ++k) acc += lens[r + k];
		r += step;
		const bool full = want_reads ? r >= want_reads : acc >= want_bases;
		if (full && (!even || !(r & 1))) { *complete = true; return r; }
	}
	return n;
}
// csrc/pair_dev.hip, csrc/align_pipeline.hip: the device's pairing stage with C linkage -- for the tests, not part of the public interface.
// bmh_pair_limit: the hits of a pair's two reads together the pairing kernel takes; the merge, its counts and the scan: see the definitions.
// bmh_pairs_device_records: what the aligner does for a batch of interleaved pairs before the host's split walk, with the insert-size statistics
// given (pes [4][5] = low, high, failed, avg, std): the single-end tail in the form the pairing kernel reads, then the pairing kernel.  Device pointers:
// reads (ASCII) / offsets, regions [n_regs][8], regions per read, frac_rep; contig_offset: host.  Out (device): d_fin [n_regs][16], d_dedup [n_regs][16]
// (the regions behind mem_sort_dedup_patch: scratch here), d_opr / d_off / d_h_rec / d_unflag [n_reads], d_todo [n_reads / 2].  popt->id0 must be even.
// Returns the record count or a negative status; waits for the stream.
extern "C" int bmh_pair_limit(void);
extern "C" int bmh_pair_merge_counts(uint32_t n_reads, const uint32_t *d_todo_pairs, uint32_t n_todo, int32_t *d_slot, const uint32_t *d_opr_dev, const int32_t *d_h_dev, const int32_t *d_uf_dev,
                                     const uint32_t *d_opr_host, const int32_t *d_h_host, const int32_t *d_uf_host, uint32_t *d_opr, int32_t *d_h, int32_t *d_uf, void *stream);
extern "C" int bmh_pair_merge_records(uint32_t n_reads, const int32_t *d_slot, const int32_t *d_fin_dev, const uint32_t *d_off_dev, const int32_t *d_fin_host, const uint32_t *d_off_host,
                                      const uint32_t *d_opr, const uint32_t *d_off, int32_t *d_fin, void *stream);
extern "C" size_t bmh_pair_scan_bytes(uint32_t n);
extern "C" int bmh_pair_scan(const uint32_t *d_in, uint32_t *d_out, uint32_t n, void *d_tmp, size_t tmp_bytes, void *stream);
extern "C" int64_t bmh_pairs_device_records(const bmh_index_t *idx, const bmh_chain_opt_t *copt, const bmh_ext_params_t *ep, const bmh_post_opt_t *popt, const bmh_pe_opt_t *pe,
                                            const double *pes, const uint8_t *d_reads, const uint32_t *d_offs, uint32_t n_reads, const int32_t *d_regs, uint64_t n_regs,
                                            const uint32_t *d_regs_per_read, const float *d_frac_rep, int n_contigs, const int64_t *contig_offset,
                                            int32_t *d_fin, int32_t *d_dedup, uint32_t *d_opr, uint32_t *d_off, int32_t *d_h_rec, int32_t *d_unflag, uint8_t *d_todo, void *stream);
// ---- interleaved pairs with mem_pair / mem_sam_pe's choices on the device (csrc/pair_dev.hip) for the pairs the mate rescue does not touch
// The host call (csrc/pair_post.cpp: bmh_finalize_pairs_split = bmh_finalize_pairs_deduped on a subset) tells the caller the insert-size statistics as
// soon as it has them (after_pestat: the caller starts the device's pair kernel), asks before its own final walk which pairs the device handed back
// (before_final: extra[n_pairs], non-zero = the host's), and walks those and the pairs the rescue touches; todo_pairs (room for n_reads / 2) receives them.
struct bmh_pairs_split_t {
	int (*after_pestat)(void *user, const double *pes /* [4][5] low, high, failed, avg, std */);
	int (*before_final)(void *user, const uint8_t **extra);
	void *user;
	uint32_t *todo_pairs; uint64_t n_todo;
	void **scratch_slot;            // optional: where the call keeps its large host arrays between calls (NULL at first; bmh_pairs_scratch_free); else the thread's
	const struct bmh_rescue_in_t *rescue_in;     // optional (csrc/pair_kernels.h): the same regions on the device -- the rescue's windows are then found there, not by a host walk
};
void bmh_pairs_scratch_free(void *p);
int64_t bmh_finalize_pairs_split(const bmh_index_t *idx, const uint8_t *d_reads, const uint32_t *d_offs, void *stream,
                                 const bmh_chain_opt_t *copt, const bmh_ext_params_t *ep, const bmh_post_opt_t *popt, const bmh_pe_opt_t *pe,
                                 int64_t l_pac, const uint8_t *pac, uint32_t n_reads, const uint8_t *reads, const uint64_t *read_offs,
                                 const uint32_t *read_lens, const int32_t *dedup_recs, const uint32_t *dedup_per_read, const float *frac_rep,
                                 int n_contigs, const int64_t *contig_offset, const int32_t *contig_len,
                                 int32_t *out, uint64_t cap, uint32_t *out_per_read, int32_t *out_h, int32_t *out_unflag, int n_threads, bmh_pairs_split_t *split);
int bmh_pair_device(const bmh_chain_opt_t *copt, const bmh_ext_params_t *ep, const bmh_post_opt_t *popt, const bmh_pe_opt_t *pe, const double *pes, int64_t l_pac,
                    int n_contigs, const int64_t *d_ctg_off, const double *d_logtab, int n_log, int32_t *d_fin, const uint32_t *d_opr, const uint32_t *d_off,
                    const float *d_frac_rep, uint32_t n_reads, int32_t *d_h_rec, int32_t *d_unflag, uint8_t *d_todo, void *stream);
// (bmh_pair_limit, the merge and the scan: C linkage, declared beside bmh_reads_last_counts above)
// bmh_finalize_regs on a subset of a batch's reads: read_ids[r] = the read's index in its batch (hash seed, record field [0]); NULL = r
int64_t bmh_finalize_regs_ids(const bmh_chain_opt_t *copt, const bmh_ext_params_t *ep, const bmh_post_opt_t *popt, int64_t l_pac,
                              const uint8_t *pac, uint32_t n_reads, const uint8_t *reads, const uint64_t *read_offs,
                              const int32_t *regs_in, const uint32_t *regs_per_read, const float *frac_rep,
                              int n_contigs, const int64_t *contig_offset,
                              int32_t *out, uint32_t *out_per_read, int n_threads, const uint32_t *read_ids);
extern "C" {
#endif
void bmh_set_error(const char *fmt, ...) __attribute__((format(printf, 1, 2)));
// Measurement knobs (csrc/c_api.hip): the value of knob `name` -- what bmh_tune_set gave it in this process, else the environment
// variable BMH_<NAME>, else dflt.  Looked up at every use (a map lookup), so that one process can sweep a knob (scripts/corun_probe.py).
int bmh_tune(const char *name, int dflt);
// wave residency trace (csrc/wtrace.h): one setter per translation unit with instrumented kernels
int bmh_wtrace_set_seed(void *buf, unsigned int *cnt, unsigned int cap);
int bmh_wtrace_set_chain(void *buf, unsigned int *cnt, unsigned int cap);
int bmh_wtrace_set_extend(void *buf, unsigned int *cnt, unsigned int cap);
#ifdef __cplusplus
}
#endif
