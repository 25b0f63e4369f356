/*
 * include/bwamem_hip.h -- device-level C ABI of the MI355X seed-and-extend library
 * (libbwamem_hip.so).  Plain pointers and sizes only; every pointer named d_* is a
 * device (HBM) pointer, everything else is host memory.
 *
 * This is the layer the reference-compatible entry points are built on:
 *   include/seed_gen.h   (replaces /root/reference/src/GPUSeed/seed_gen.h:92-106)
 *   include/gasal_ext.h  (replaces the GASAL2 calls of /root/reference/src/bwamem.c:1102-1167,
 *                         2106-2211 and src/fastmap.c:417-534)
 * and the layer bench.py / the multi-GPU launcher use so that inputs are already
 * resident in HBM when timing starts.
 *
 * Error behaviour: functions returning int return 0 on success and a negative
 * BMH_E* code on failure; bmh_last_error() gives the message.  Nothing here
 * falls back to a CPU implementation: without a HIP device every call fails.
 */
#ifndef BWAMEM_HIP_H
#define BWAMEM_HIP_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define BMH_OK          0
#define BMH_ENODEV     -1   /* no HIP device / HIP runtime error */
#define BMH_EINVAL     -2   /* bad argument */
#define BMH_ECAPACITY  -3   /* a workspace capacity was exceeded (reference: exit(), seed_gen.cu:2037-2042) */
#define BMH_ENOMEM     -4

const char *bmh_last_error(void);
int bmh_device_count(void);
int bmh_set_device(int dev);

/* ------------------------------------------------------------------ index */

/* FMD index resident in HBM.  The arrays that cross this interface have the reference's
 * GPU layout (seed_gen.cu:28-48; seed_gen.h:21-33 bwt_t_gpu): blocks {u32 occ[4]; u32 bwt[4]}.
 * A handle keeps the blocks re-encoded as {u32 occ[4]; u64 low bit plane; u64 high bit plane}
 * (same 32 bytes per 64 symbols; csrc/fmd_dev.h) -- bmh_index_upload converts its device copy
 * in place, bmh_index_from_device makes its own converted copy (seq_len / 2 bytes of HBM) and
 * leaves the caller's buffer as it is. */
typedef struct bmh_index bmh_index_t;

/* host arrays -> HBM (replaces gpu_cpy_wrapper, seed_gen.cu:1524-1556).
 * bwt_words: interleaved occ/bwt blocks, n_words u32; sa: n_sa u32 samples with
 * sa[0] ignored; sa_bits: n_sa/32+1 words; pac (optional, may be NULL): 2-bit
 * forward strand, l_pac bases. */
bmh_index_t *bmh_index_upload(uint64_t primary, const uint64_t L2[5], uint64_t seq_len,
                              const uint32_t *bwt_words, uint64_t n_words, int sa_intv,
                              const uint32_t *sa, uint64_t n_sa, const uint32_t *sa_bits,
                              const uint8_t *pac, uint64_t l_pac);
/* wrap arrays that already live in HBM (e.g. received by an RCCL broadcast);
 * the index does not own them.  d_pac (optional): 4-byte aligned, readable for
 * l_pac/4 + 9 bytes (the kernels fetch the text in aligned words).  With the
 * text resident the seeding kernels stop ranking once an interval holds one
 * suffix and compare the read with the text instead. */
bmh_index_t *bmh_index_from_device(uint64_t primary, const uint64_t L2[5], uint64_t seq_len,
                                   const uint32_t *d_bwt_words, uint64_t n_words, int sa_intv,
                                   const uint32_t *d_sa, uint64_t n_sa, const uint32_t *d_sa_bits,
                                   const uint8_t *d_pac, uint64_t l_pac);
void bmh_index_free(bmh_index_t *idx);
/* A handle with the 2-bit text also holds a bitmap of the K-mers that occur in the indexed text fwd . revcomp(fwd)
 * (csrc/kmer_bits.hip): K is the smallest with 4^K >= 8 seq_len, at most 18 (8 GiB at hg38 scale); key of a K-mer = its
 * symbol j at bits 2j+1:2j, bit (key & 31) of word (key >> 5).  It is built on the device when the handle is made -- by
 * every function that makes one, on the handle's own device -- and freed with it.  With min_seed_len >= K the forward
 * search of bmh_seed_batch skips candidates that cannot reach min_seed_len; seeds are the same with and without it.
 * No text, BMH_SEED_KBITS=0 in the environment when the handle is made, or no memory for it: the handle has none.
 * bmh_index_kbits_info: *k = K (0: none), *d_bits = the bitmap in HBM (NULL: none), *n_words = its 32-bit words. */
int bmh_index_kbits_info(const bmh_index_t *idx, int *k, const uint32_t **d_bits, uint64_t *n_words);
/* Rank primitives at n given rows (d_rows, d_out: device memory), asynchronous on `stream`:
 *   what = 0: d_out[4 i + c] = Occ(rows[i], c), c = A,C,G,T  (bwt_occ4, src/bwt.c:309-330; rows -1 and seq_len allowed)
 *   what = 1: d_out[i] = LF(rows[i])                         (bwt_invPsi, src/bwt.c:64-70)
 *   what = 2: d_out[i] = SA[rows[i]]                         (bwt_sa, src/bwt.c:105-115)
 * rows of 1 / 2 must lie in [0, seq_len]. */
int bmh_index_probe(const bmh_index_t *idx, const uint64_t *d_rows, uint64_t n, int what, uint64_t *d_out, void *stream);

/* ---- several GPUs of one node from C: the index on every device, the reads sharded, one host worker thread per device
 * (the reference has no multi-GPU mode at all: gasal_set_device is commented out at src/fastmap.c:143).
 * bmh_index_replicate copies an index that lives on src_device into fresh allocations on dst_device (device to device: xGMI
 * between the GPUs of a node; src_device == dst_device makes a second copy on the same GPU).  The copy owns its arrays (free it
 * with bmh_index_free while dst_device is current).  bmh_shard_range: the contiguous part [lo, hi) of n reads that worker `rank`
 * of `world` takes, cut at multiples of `multiple` (2 keeps interleaved pairs together).
 * The drop-in entry points use them when BMH_DEVICES=N is set: seed_gpu() sends the batches of the read file round-robin to N
 * worker threads, one per device, and concatenates their seeds in file order; the gasal_gpu_storage_t objects of
 * gasal_init_streams are spread over the N devices.  With fewer physical devices than N several workers share one. */
int bmh_index_replicate(const bmh_index_t *src, int src_device, int dst_device, bmh_index_t **out);

/* ---- the same with RCCL over xGMI (csrc/rccl_bcast.hip).  RCCL is resolved at run time -- the symbols already in the process (a
 * host linked with -lrccl), then $BMH_RCCL_LIB, then librccl.so.1 of the loader path -- because a communicator is only valid in
 * the library instance that made it; bmh_rccl_where() names the instance in use (NULL: none found, bmh_last_error says why).
 * One process per GPU: rank 0 calls bmh_rccl_unique_id and hands the 128 bytes to the others by its own means (a file, MPI, a
 * socket), every rank calls bmh_rccl_comm_init_rank on its device and then bmh_index_broadcast_rccl: the root passes its index
 * (out == NULL: send only; out != NULL: it receives a fresh copy like the others), the others receive theirs in *out (owned:
 * bmh_index_free).  One 128-byte header, then the blocks (native layout), the suffix array, its high bits and the 2-bit text in
 * ONE grouped broadcast, in pieces of at most 1 GiB, on `stream`; returns when the arrays have arrived.
 * One process, n devices: bmh_index_replicate_all makes out[k] the index on devices[k] (src itself on src_device; duplicates in
 * the list share a copy) with ncclCommInitAll and the same grouped broadcast; *used_rccl (optional) says whether RCCL carried it
 * or the hipMemcpyPeer fallback did (RCCL not found, or BMH_REPLICATE=peer).  BMH_DEVICES=N of the drop-in uses this. */
const char *bmh_rccl_where(void);
int bmh_rccl_unique_id(void *id128);
int bmh_rccl_comm_init_rank(void **comm, int nranks, const void *id128, int rank);
void bmh_rccl_comm_destroy(void *comm);
int bmh_index_broadcast_rccl(void *comm, int root, const bmh_index_t *src, bmh_index_t **out, void *stream);
int bmh_index_replicate_all(const bmh_index_t *src, int src_device, const int *devices, int n, bmh_index_t **out, int *used_rccl);
void bmh_shard_range(uint64_t n, int rank, int world, uint32_t multiple, uint64_t *lo, uint64_t *hi);

/* Replaces the suffix-array samples by denser ones (every new_intv-th row, a power of two; a no-op if the index is that
 * dense already), computed on the device from the existing ones: same values, fewer LF steps per located seed, more HBM
 * (4.125 bytes per sample).  The reference's files hold every 16th row (src/bwtindex.c:324). */
int bmh_index_densify_sa(bmh_index_t *idx, int new_intv);

/* Builds the FMD index of fwd . revcomp(fwd) ON THE DEVICE from the 2-bit forward strand (d_pac: l_pac bases, 4 per byte,
 * first base in the top bits -- the .pac body; l_pac < 2^32, i.e. texts up to 2^33 symbols: hg38 has 6.2e9).  Replaces the
 * reference's offline host passes (bwa_index/bwtindex.c:287-358 bwtsw construction, :174-197 GPU re-blocking,
 * bwa_index/bwt.c:63-148 sampled suffix array) with the same values: the outputs are exactly what bmh_index_from_device
 * takes and, copied to the host, the bodies of the reference's .bwt / .sa files.
 * Caller-allocated device outputs (seq_len = 2 l_pac):
 *   d_bwt_words  (ceil(seq_len/64) + 1) * 8 words, 32-byte aligned: blocks {u32 occ[4]; u32 bwt[4]}, then one block whose occ
 *                is the totals;  d_sa  n_sa = (seq_len + sa_intv) / sa_intv words (sa[0] = 0xFFFFFFFF);  d_sa_bits  n_sa/32 + 1 words.
 * sa_intv: power of two; 16 = what the reference's files hold, 1 = the whole suffix array (what the seeding kernels like best).
 * flags: BMH_BUILD_VERIFY checks the finished suffix array completely (every adjacent pair of rows compared symbol by symbol,
 * SA a permutation) before anything is written.  Uses about 24 bytes of HBM per symbol of seq_len while it runs (175 GB for
 * hg38) and synchronises the device.  stats (optional) reports what happened. */
#define BMH_BUILD_VERIFY 1
typedef struct {
	int round0_passes, doubling_rounds, verified;
	uint64_t unresolved_after_round0;
	double round0_seconds, sa_seconds, verify_seconds, total_seconds;
} bmh_build_stats_t;
int bmh_index_build(const uint8_t *d_pac, uint64_t l_pac, int sa_intv, uint32_t *d_bwt_words, uint32_t *d_sa, uint32_t *d_sa_bits,
                    uint64_t *primary_out, uint64_t L2_out[5], int flags, bmh_build_stats_t *stats);

/* `bwa index` on the device (csrc/fasta_pack.hip): a FASTA file, plain or gzip (by its magic bytes; zlib is loaded with
 * dlopen("libz.so.1")), in; prefix.{bwt,sa,pac,ann,amb} out, byte for byte what the reference's two-pass build writes
 * (bwa_index/bntseq.c bns_fasta2bntseq over kseq_read, then bmh_index_build).  The file is streamed in chunks of chunk_bytes
 * (0: 256 MiB; 64 .. 2^31) through pinned double buffers and packed into the 2-bit forward strand on the device; the
 * packer's buffers (about 66 bytes of HBM per chunk byte) are freed before the builder runs.  sa_intv: a power of two (the
 * builder's; `bwa index -r` takes any value).  flags: BMH_BUILD_VERIFY.  Refused with BMH_EINVAL and nothing written under
 * the final names: a file with no record, with only empty records, with a line that starts with '+' (FASTQ), or with a
 * sequence byte 0 or >= 128; an unreadable file; a .gz without zlib.  More than 2^32 - 1 bases: BMH_ECAPACITY.  The files
 * are written under temporary names and renamed at the end.  stats (optional) reports what happened. */
typedef struct {
	uint64_t n_contigs, n_holes, l_pac, n_ambig, file_bytes;
	double read_seconds;     /* reading / inflating the file (the part not hidden behind the device's work) */
	double h2d_seconds, pack_seconds, build_seconds, write_seconds, total_seconds;
	int verified;
} bmh_index_fasta_stats_t;
int bmh_index_fasta(const char *fa_path, const char *prefix, int sa_intv, int flags, size_t chunk_bytes, bmh_index_fasta_stats_t *stats);
/* The packing step alone: d_pac (device, pac_bytes >= (l_pac+3)/4 + 64, zero beyond the text) and the host tables of the
 * .ann / .amb -- per contig its name and comment (NUL-terminated at name_off / comment_off; an empty comment is written
 * "(null)"), offset, length and holes; per hole its offset, length and byte.  Free with bmh_fasta_packed_free. */
typedef struct {
	uint8_t *d_pac; uint64_t pac_bytes, l_pac, n_ambig;
	int32_t n_contigs; char *names, *comments; uint64_t *name_off, *comment_off; int64_t *offsets, *lens; int32_t *n_ambs;
	int64_t n_holes; int64_t *hole_off, *hole_len; uint8_t *hole_char;
} bmh_fasta_packed_t;
int bmh_fasta_pack(const char *fa_path, size_t chunk_bytes, bmh_fasta_packed_t *out, bmh_index_fasta_stats_t *stats);
void bmh_fasta_packed_free(bmh_fasta_packed_t *p);

/* ---------------------------------------------------------------- seeding */

/* Workspace for batches of up to max_reads reads / max_bases bases.
 * max_cands bounds SMEM candidates per batch (0 = default guess: 16 per read + 0.4 per base; the hard
 * upper bound, which never fails, is one per base -- bmh_seed_batch returns BMH_ECAPACITY beyond the
 * capacity); max_occ sizes the arrays of located occurrences (0 = 64 per read): a batch that needs
 * more gets larger arrays inside bmh_seed_batch. */
typedef struct bmh_seed_ws bmh_seed_ws_t;
bmh_seed_ws_t *bmh_seed_ws_create(uint32_t max_reads, uint64_t max_bases, uint64_t max_cands, uint64_t max_occ);
void bmh_seed_ws_free(bmh_seed_ws_t *ws);

/* Seeds of one batch, in HBM, in the reference's mem_seed_v_gpu layout
 * (seed_gen.h:68-75): per read SMEMs by end ascending, occurrences by SA row
 * ascending; score = #occurrences at the first slot of each SMEM group, 0 in
 * the others.  Pointers stay valid until the next call on the same workspace.
 *
 * A workspace with a sample set (bmh_seed_ws_set_sample, below) writes a SAMPLED batch: the layout, the counts and every group
 * head (d_qbeg, d_score = s) are the complete batch's, but of a group of s > max_occ slots only the slots mem_chain reads with
 * that max_occ hold values -- u = j * (s / max_occ), j < min(ceil(s / (s / max_occ)), max_occ) (src/bwamem.c:430-436); the
 * slots between them are not written.  bmh_chain_batch / bmh_chain_extend_merge take such a batch as it is when their max_occ
 * is the sample's and complete it first when not; whoever reads the arrays another way calls bmh_seeds_locate_all first. */
typedef struct {
	uint64_t n_seeds;            /* occurrences laid out in the batch (all located unless the batch is sampled) */
	uint64_t n_smems;            /* SMEM groups */
	uint64_t n_cands;            /* forward candidates examined */
	const uint64_t *d_rbeg;      /* [n_seeds] position in the fwd+revcomp text */
	const int32_t *d_qbeg;       /* [n_seeds][2] = {begin, end} in the read */
	const uint32_t *d_score;     /* [n_seeds] */
	const uint32_t *d_n_ref_pos; /* [n_reads] occurrences per read */
	const uint32_t *d_prefix;    /* [n_reads] exclusive scan of d_n_ref_pos */
} bmh_seeds_t;

/* d_reads: ASCII bases of all reads back to back (no separators), d_offs/d_lens
 * per read (what the reference copies to the GPU, seed_gen.cu:1841-1843).
 * stream: a hipStream_t (NULL = default stream).  Synchronises the stream: the call waits on the host for what the stream
 * holds, runs its kernels on a stream of the highest priority that the workspace owns (beside another batch's extension kernels
 * the seeding waves -- which wait on HBM most of the time -- then take the wave slots that become free; BMH_SEED_PRIO=normal in the
 * environment when the workspace is created: on `stream` itself), and leaves `stream` waiting for them: work queued on `stream`
 * afterwards sees the seeds. */
int bmh_seed_batch(bmh_seed_ws_t *ws, const bmh_index_t *idx, const uint8_t *d_reads,
                   const uint32_t *d_offs, const uint32_t *d_lens, uint32_t n_reads,
                   int min_seed_len, void *stream, bmh_seeds_t *out);

/* BWA-MEM's second and third seeding rounds (mem_collect_intv with re_seed, src/bwamem.c:266-297; gase_aln -g).
 * Round 2 re-seeds from the middle of every SMEM of at least (int)(min_seed_len * split_factor + .499) bases with at most split_width
 * occurrences (bwt_smem1 with min_intv = occurrences + 1); round 3 (max_mem_intv > 0) scans the read for the shortest seeds of more
 * than min_seed_len bases with fewer than max_mem_intv occurrences (bwt_seed_strategy1).  The groups of all three rounds are merged
 * per read by (begin, end), duplicates kept, in the layout of bmh_seeds_t. */
typedef struct { int enable; float split_factor; int split_width; int max_mem_intv; } bmh_reseed_opt_t;
void bmh_reseed_opt_default(bmh_reseed_opt_t *o);      /* 0 / 1.5 / 10 / 20, as mem_opt_init (src/bwamem.c:115-125) */
/* bmh_seed_batch with the re-seeding rounds; opt NULL or opt->enable == 0: exactly bmh_seed_batch. */
int bmh_seed_batch_reseed(bmh_seed_ws_t *ws, const bmh_index_t *idx, const uint8_t *d_reads,
                          const uint32_t *d_offs, const uint32_t *d_lens, uint32_t n_reads,
                          int min_seed_len, const bmh_reseed_opt_t *opt, void *stream, bmh_seeds_t *out);
/* Which path the calling thread's last bmh_seed_batch_reseed took: out[0] = round-2 tasks, out[1] = tasks whose forward list did not fit
 * the first launch's column (knob RESEED_CAP, 32 entries) and ran again in the second, out[2..4] = seed groups of rounds 1, 2 and 3, out[5] = rank steps
 * (interval extensions) of round 2's lanes in both launches, out[6] = of round 3's.  All 0 before any call, after a call with re-seeding off, and
 * after one that failed before the merge.  For tests. */
int bmh_reseed_last_counts(uint64_t out[7]);

/* Sampled locate.  max_occ > 0: the batches that follow locate, of every SMEM group, only the occurrences that chaining with this
 * max_occ (bmh_chain_opt_t) reads -- see bmh_seeds_t -- where the index holds the whole suffix array (sa_intv 1); 0 (the default):
 * every occurrence.  Batches of an index with sa_intv > 1, of bmh_seed_batch_reseed with re-seeding on and of the BMH_SEED_FUSED
 * form are complete whatever the setting. */
int bmh_seed_ws_set_sample(bmh_seed_ws_t *ws, uint32_t max_occ);
/* How the arrays of `seeds` stand: the max_occ they were sampled with, 0 when every slot is filled (a complete batch, a completed
 * one, or a record whose arrays belong to no live workspace, e.g. one built by hand). */
uint32_t bmh_seeds_sample_state(const bmh_seeds_t *seeds);
/* Fills every slot of a sampled batch (the full expand + locate over what its workspace kept of it; valid until the workspace's next
 * batch; the index must still be alive) and waits for it.  Nothing to do, and BMH_OK, for seeds in the state 0. */
int bmh_seeds_locate_all(const bmh_seeds_t *seeds, void *stream);

/* per-kernel time of the last bmh_seed_batch, in ms (HIP events on the launch stream):
 * [0]=pack [1]=forward [2]=scatter+backward [3]=filter+scans [4]=expand [5]=locate [6]=total
 * (a sampled batch: [4]=the one pass that writes and locates the sampled slots, [5]=no kernel, the microseconds between
 * two event records, never exactly 0;
 * with BMH_SEED_FUSED=1: [1]=fused forward+backward [2]=sort of the SMEMs [3]=gather+scans) */
void bmh_seed_last_timing(const bmh_seed_ws_t *ws, float ms[7]);

/* Calibration: n_lanes lanes each gather `iters` random 32-byte index blocks (dependent != 0:
 * each address depends on the previous block, like a rank walk).  *ms = kernel time.  Known
 * byte count = n_lanes * iters * 32; used to calibrate rocprofv3 FETCH_SIZE for this access
 * pattern and to measure the practical random-gather ceiling of the chip. */
int bmh_calib_gather(const bmh_index_t *idx, uint64_t n_lanes, int iters, int dependent, void *stream, float *ms);

/* Calibration of the integer-VALU roofline the extension kernels are held against: waves_per_simd resident waves on every
 * SIMD execute `iters` rounds of 128 instructions of one kind -- mode 0: independent v_max_i32 / v_add_u32 (the issue ceiling),
 * 1: one dependent chain, 2: dependent DPP row_shr max (the scans), 3: independent DPP, 4: packed 16-bit add / max,
 * 5: v_bfe_i32, 6: v_fma_f32, 7: v_pk_fma_f32 (two fp32 lanes per instruction: the form the chip's 157 TFLOP/s vector figure
 * needs), 8: the packed DP kernels' own mix (v_pk_mad / sub / max / min / add_u16, v_perm_b32, v_and_b32).
 * *ms = kernel time, *lane_ops = 64 x 128 x iters per wave, summed over the waves (instructions x 64: a packed instruction
 * counts once).  bmh_calib_valu_placed also returns, for every wave of the timed launch, (XCC_ID << 32 | HW_ID) in place[]
 * (host memory for 4 x 256-thread-blocks words; *n_place = how many): which SIMD of which CU of which XCD the wave ran on. */
int bmh_calib_valu(int mode, int waves_per_simd, int iters, void *stream, float *ms, double *lane_ops);
int bmh_calib_valu_placed(int mode, int waves_per_simd, int iters, void *stream, float *ms, double *lane_ops,
                          unsigned long long *place, unsigned *n_place);
/* The shader clock (MHz) and the shader cycles per wave64 instruction of one wave during the calling thread's last bmh_calib_valu[_placed]
 * launch, measured inside the kernel (s_memtime over s_memrealtime); BMH_EINVAL before any calibration. */
int bmh_calib_last_clock(double *mhz, double *cycles_per_instr);

/* -------------------------------------------------------------- extension */

/* Scoring of ksw_extend2 (src/ksw.c:864) as used by the GPU pipeline
 * (src/bwamem.c:1887-1890): mat[i][j] = a / -b / -1 against code 4
 * (src/bwa.c:99-108), affine gaps, end_bonus = pen_clip5, zdrop (0 = off). */
typedef struct {
	int a, b;
	int o_del, e_del, o_ins, e_ins;
	int zdrop, end_bonus;
} bmh_ext_params_t;

/* n extensions: query/target bases are codes 0..4, one byte per base, at
 * d_q + d_qoff[i] (d_qlen[i] bases) and d_t + d_toff[i] (d_tlen[i]);
 * d_h0[i] = seed score.  Results (src/bwamem.c:1893-1901 rule applied):
 * d_out[3*i+0..2] = {aln_score, query_end, target_end}; if d_raw != NULL also
 * d_raw[6*i..] = {score, qle, tle, gtle, gscore, max_off} of ksw_extend2.
 * Asynchronous on stream. */
int bmh_extend_batch(const uint8_t *d_q, const uint32_t *d_qoff, const uint32_t *d_qlen,
                     const uint8_t *d_t, const uint32_t *d_toff, const uint32_t *d_tlen,
                     const uint32_t *d_h0, uint32_t n, const bmh_ext_params_t *p,
                     int32_t *d_out, int32_t *d_raw, void *stream);

/* Queries longer than 768 bases are not supported by the DP kernels (the reference's GASAL2 build has a compile-time
 * MAX_SEQ_LEN too, README.md:38): such a job gets INT32_MIN in all three outputs and is counted; this returns the count for the
 * calling thread's last bmh_extend_batch (waits for it; -1 on a HIP error).  The reference-compatible layer (gasal_aln_async)
 * refuses such a batch up front; bmh_chain_batch only admits reads up to 700 bases, whose flanks always fit. */
int64_t bmh_extend_last_unsupported(void);

/* Jobs per kernel class of the calling thread's last bmh_extend_batch[_long] (waits for it): sizes[c] for c < min(cap, number of
 * classes); returns the number of classes (0 before any batch).  Class 0 = unsupported, 1..18 = 16-lane rows, 19..26 = wide
 * kernel, 27 = decided without DP (closed form), 28..48 = packed 16-bit kernels, 49..53 = long-query kernel.  For tests. */
int bmh_extend_last_class_sizes(uint32_t *sizes, int cap);

/* Long queries, opt-in: bmh_extend_batch, except that jobs whose query has 769 .. min(max_qlen, BMH_EXT_LONG_MAX) bases (max_qlen 0:
 * BMH_EXT_LONG_MAX) run on the long-query kernel (one workgroup per alignment; same contract, results bit-identical to ksw_extend2
 * without a band).  Jobs of at most 768 bases take exactly the kernels of bmh_extend_batch; longer ones than the cap get INT32_MIN
 * and are counted by bmh_extend_last_unsupported. */
#define BMH_EXT_LONG_MAX 16384
int bmh_extend_batch_long(const uint8_t *d_q, const uint32_t *d_qoff, const uint32_t *d_qlen,
                          const uint8_t *d_t, const uint32_t *d_toff, const uint32_t *d_tlen,
                          const uint32_t *d_h0, uint32_t n, const bmh_ext_params_t *p, uint32_t max_qlen,
                          int32_t *d_out, int32_t *d_raw, void *stream);

/* Jobs whose scores fit 16 bits (h0 + qlen*a < 4096; scoring with 1 <= b, a + b <= 255) and whose sides fit a packed class -- qlen <= 128
 * with tlen <= 384 (4 lanes per job, 16 jobs per wave; qlen 129..136 too while h0 + qlen*a < 2048: the 17-pair class), qlen <= 256
 * with tlen <= 512 (8 lanes, 8 jobs per wave), qlen <= 288 with tlen <= 640 (16 lanes, 4 jobs per wave) -- run on the packed 16-bit
 * kernels (two DP columns per register), everything else on the 32-bit kernels; results are identical.  on = 0 sends every job to the 32-bit kernels (tests, A/B timing).  Process-wide; returns the previous setting. */
int bmh_extend_set_packed(int on);

/* Measurement knobs of the library (each documented where it is read): knob NAME takes the value given here, else
 * the environment variable BMH_<NAME>, else its default; clear != 0 forgets a value set earlier.  Process-wide; for A/B sweeps inside
 * one process (scripts/corun_probe.py).  No reference counterpart. */
int bmh_tune_set(const char *name, int value, int clear);
/* Wave residency trace (measurement; csrc/wtrace.h): between start and stop every wave of the seeding, chaining and packed extension
 * kernels leaves a 32-byte record {u32 kernel id, HW_ID, XCC_ID, aux; u64 t0, t1 in 100 MHz ticks}; stop waits for the device, copies up to
 * max_recs records and returns how many waves reported.  scripts/wave_residency.py turns them into waves of each kernel per SIMD over time. */
int bmh_wtrace_start(uint32_t cap);
int64_t bmh_wtrace_stop(void *out, uint32_t max_recs);
uint32_t bmh_wtrace_kept(void);          /* records the last bmh_wtrace_stop copied out */

/* bmh_extend_batch keeps scratch (the sorted job list, four side streams, events) per (device, stream) and reuses it across calls.
 * Call this before destroying a stream that ran extensions (stream idle, its device current); without it the entry stays until the
 * process ends and a recycled stream handle would inherit it.  One stream must not run extensions from two host threads at once.
 * bmh_finalize_regs_device and bmh_finalize_pairs_dev / bmh_matesw_batch_device keep scratch by the same rule (device buffers, side
 * streams, events, pinned words per (device, stream); ONE host thread per stream at a time): bmh_finalize_release and
 * bmh_matesw_release free theirs, and bmh_extend_release calls both. */
void bmh_extend_release(void *stream);
void bmh_finalize_release(void *stream);
void bmh_matesw_release(void *stream);

/* device time in ms of the DP kernels launched by the calling thread's last
 * bmh_extend_batch (HIP events on that call's stream; waits for them). */
float bmh_extend_last_ms(void);

/* ------------------------------------------------- host job builder */

/* The options of mem_opt_t this stage reads; bmh_chain_opt_default() = mem_opt_init()
 * (src/bwamem.c:101-146). */
typedef struct {
	int a, b, o_del, e_del, o_ins, e_ins, w;
	int min_seed_len, max_occ, max_chain_gap, min_chain_weight, max_chain_extend;
	float mask_level, drop_ratio;
	/* ALT contigs (the reference reads <prefix>.alt, src/bntseq.c:179-200; bns->anns[rid].is_alt): contig_is_alt[n_contigs] in HOST
	 * memory, NULL = none.  Read by bmh_build_jobs (mem_chain_flt ignores an overlap whose kept chain is ALT while the current one is
	 * not, src/bwamem.c:518); the device job builder takes the flags through bmh_chain_set_alt instead. */
	const uint8_t *contig_is_alt;
} bmh_chain_opt_t;
void bmh_chain_opt_default(bmh_chain_opt_t *o);

/* seeds (host copies of the mem_seed_v_gpu arrays) -> chains -> filtered chains -> extension jobs,
 * restating mem_chain / mem_chain_flt / mem_chain2aln (src/bwamem.c:404-477, 487-559, 1170-1479).
 * reads: nt4 codes; pac: 2-bit forward strand (the .pac file body); contigs: n_contigs offsets/lens
 * (n_contigs <= 1: one sequence of l_pac bases).  Jobs come out per read, per region, LEFT then RIGHT.
 * Includes the seed filter mem_flt_chained_seeds + mem_seed_sw (src/bwamem.c:970-991, 774-807), which the reference runs when
 * (min_chain_weight ? 1.1f * min_chain_weight : 5.5 ln l_query) <= 0.05f * l_query -- reads beyond ~730 bp, or a small explicit
 * -W: every seed of the kept chains is re-scored by a local alignment of its neighbourhood (ksw_align2 semantics) and weak
 * seeds are dropped.  bmh_chain_batch runs the same filter on the device (round 3) for the reads it admits (up to 700 bases, i.e.
 * whenever a small -W switches it on); a batch with a longer read is refused there (BMH_EINVAL) and belongs here. */
typedef struct bmh_jobs bmh_jobs_t;
bmh_jobs_t *bmh_build_jobs(const bmh_chain_opt_t *opt, int64_t l_pac, const uint8_t *pac, int n_contigs,
                           const int64_t *contig_offset, const int32_t *contig_len, uint32_t n_reads,
                           const uint8_t *reads, const uint64_t *read_offs, const uint32_t *read_lens,
                           const uint64_t *rbeg, const int32_t *qbeg, const uint32_t *score,
                           const uint32_t *n_ref_pos, const uint32_t *prefix, int n_threads);
void bmh_jobs_free(bmh_jobs_t *j);
void bmh_jobs_sizes(const bmh_jobs_t *j, uint64_t *n_jobs, uint64_t *n_regs, uint64_t *q_bytes, uint64_t *t_bytes);
/* borrowed pointers into the job batch (valid until bmh_jobs_free): the bmh_extend_batch inputs, the
 * read / region / side (0 left, 1 right) of every job, and the number of regions of every read */
void bmh_jobs_arrays(const bmh_jobs_t *j, const uint8_t **q, const uint32_t **qoff, const uint32_t **qlen,
                     const uint8_t **t, const uint32_t **toff, const uint32_t **tlen, const uint32_t **h0,
                     const uint32_t **job_read, const uint32_t **job_reg, const uint32_t **job_side,
                     const uint32_t **regs_per_read);
/* extension results -> alignment regions (src/bwamem.c:2297-2303): regs_out[n_regs][8] =
 * {read, score, qb, qe, rb_lo, rb_hi, re_lo, re_hi} */
int bmh_merge_regs(const bmh_jobs_t *j, const int32_t *out3, int32_t *regs_out);

/* per read: the frac_rep of its chains (mem_chain, src/bwamem.c:415-459), needed by the MAPQ estimate */
const float *bmh_jobs_frac_rep(const bmh_jobs_t *j);

/* ------------------------------------------------- after the extension: which regions are reported (SURVEY 8f rank 1 tail, rank 4) */

/* the options of mem_opt_t this stage reads beyond bmh_chain_opt_t / bmh_ext_params_t; bmh_post_opt_default() = mem_opt_init() */
typedef struct {
	int T;                      /* minimum score of a reported alignment (30) */
	float mask_level_redun;     /* 0.95 */
	float mapQ_coef_len;        /* 50 */
	int mapQ_coef_fac;          /* (int)log(50) = 3 */
	int flag_all;               /* MEM_F_ALL (-a): report secondary alignments too */
	int64_t id0;                /* index of the batch's first read in the run (n_processed): seeds the tie-break hash */
	float XA_drop_ratio;        /* 0.80: secondary hits scoring at least this share of their primary go to its XA tag */
	int max_XA_hits;            /* 5: ... when there are no more than this many */
	int no_multi;               /* MEM_F_NO_MULTI (-M): shorter split hits are flagged secondary (0x100) instead of supplementary */
	int softclip;               /* MEM_F_SOFTCLIP (-Y): soft clips on every record (no hard clips on the later ones) */
	int max_XA_hits_alt;        /* 200: ... or this many when one of them lies on an ALT contig (-h INT,INT) */
	/* ALT contigs: contig_is_alt[n_contigs] in HOST memory, NULL = none (src/bwamem.c:571-574,702,721-760,1540,1578,1663,1742,1755,
	 * 2323; src/bwamem_extra.c:106-150).  With a table that flags at least one sequence the records change in two places:
	 * [11] holds secondary_all (the parent of the FIRST marking round over all hits, which the XA tag goes by) instead of sub_n, and
	 * [15] = reported | is_alt << 1 | alt_sc << 2 ([12] secondary is INT_MAX for an ALT hit that has a parent, as in the reference).
	 * bmh_finalize_regs and bmh_finalize_regs_device both take the table (the device form uploads it; the second marking round,
	 * secondary_all and alt_sc are in csrc/regs_core.h and the wave classes of csrc/regs_kernels.hip): same records. */
	const uint8_t *contig_is_alt;
	/* read group (-R: bwa_set_rg, src/bwa.c:425-452): the ID of the @RG line, NUL-terminated, in HOST memory, at most 255 characters; NULL or empty = none.  Every
	 * record -- the unmapped ones too -- gets RG:Z:<id> behind AS / XS and in front of SA (mem_aln2sam, src/bwamem.c:1631-1634); the caller writes the @RG header line. */
	const char *rg_id;
	/* -C: the read's header comment, a tab in front, at the end of every record -- the unmapped ones too (mem_aln2sam, src/bwamem.c:1670-1673).
	 * 0 (the default): none.  The writers take the comments from their own arguments (bmh_format_sam_ex, bmh_sam_dev_t, bmh_read_set_t). */
	int copy_comment;
} bmh_post_opt_t;
void bmh_post_opt_default(bmh_post_opt_t *o);

/* Per read: mem_sort_dedup_patch (redundant regions removed, colinear ones merged when a global alignment across both
 * scores well enough), mem_mark_primary_se (primary / secondary, sub-optimal score), mem_approx_mapq_se and the
 * selection of mem_reg2sam (src/bwamem.c:620-680, 685-760, 1690-1717, 1721-1770).  Host code, like the reference's.
 * regs_in[..][8] = bmh_merge_regs / bmh_chain_merge layout, grouped by read (regs_per_read); frac_rep per read.
 * out[..][16] = {read, score, qb, qe, rb_lo, rb_hi, re_lo, re_hi, truesc, w, sub (XS), sub_n, secondary (index within
 * the read's output, -1 = primary line), MAPQ, flag (0x100 secondary, 0x800 supplementary), reported (0/1)} in the
 * reference's order, capacity = the number of input regions; out_per_read[n_reads].  Returns the number of output
 * regions or a negative BMH_E* code.  contig_offset: start of every sequence in the packed reference (bns->anns[i].offset;
 * n_contigs <= 1: one sequence).  ALT contigs: popt->contig_is_alt (see bmh_post_opt_t). */
int64_t bmh_finalize_regs(const bmh_chain_opt_t *copt, const bmh_ext_params_t *ep, const bmh_post_opt_t *popt, int64_t l_pac,
                          const uint8_t *pac, uint32_t n_reads, const uint8_t *reads, const uint64_t *read_offs,
                          const int32_t *regs_in, const uint32_t *regs_per_read, const float *frac_rep,
                          int n_contigs, const int64_t *contig_offset,
                          int32_t *out, uint32_t *out_per_read, int n_threads);

/* The same tail ON THE DEVICE (csrc/regs_kernels.hip; reads -> reportable alignments without leaving HBM): every pointer except
 * contig_offset is device memory.  d_regs[n_regs][8], d_regs_per_read, d_frac_rep: what bmh_chain_merge / bmh_chain_extend_merge
 * left (bmh_dev_jobs_t); d_reads / d_offs: the batch's ASCII reads; the index must carry the 2-bit reference.  d_out[n_regs][16]:
 * the records of bmh_finalize_regs, in the same order; d_out_per_read[n_reads].  Returns their number or a negative BMH_E* code;
 * waits for the stream.  Same results as bmh_finalize_regs, record for record (the logarithms of the MAPQ formula come from a
 * table computed by the host's libm).  Interleaved pairs still go through bmh_finalize_pairs. */
int64_t bmh_finalize_regs_device(const bmh_index_t *idx, const bmh_chain_opt_t *copt, const bmh_ext_params_t *ep, const bmh_post_opt_t *popt,
                                 const uint8_t *d_reads, const uint32_t *d_offs, uint32_t n_reads,
                                 const int32_t *d_regs, uint64_t n_regs, const uint32_t *d_regs_per_read, const float *d_frac_rep,
                                 int n_contigs, const int64_t *contig_offset, int32_t *d_out, uint32_t *d_out_per_read, void *stream);
float bmh_finalize_regs_device_last_ms(void);       /* device time of the thread's last bmh_finalize_regs_device (HIP events) */
/* Which form took which read in the thread's last bmh_finalize_regs_device / bmh_dedup_regs_device: out[c] = the reads handed to the wave
 * kernel of class c (up to 32 / 128 / 256 / 512 / more regions; class 0 includes the reads of at most 8 regions whose patch test reached
 * its global alignment), every other read with regions was finished by the lane kernel.  0, or BMH_EINVAL without such a call.  For tests. */
int bmh_finalize_regs_device_last_classes(uint32_t out[5]);

/* SAM records of single-end reads (mem_aln2sam, src/bwamem.c:1506-1683; XA tag: mem_gen_alt, src/bwamem_extra.c:97-150).
 * bmh_sam_need_cigar marks (need[i] = 1) the records of bmh_finalize_regs that must go through bmh_cigar_batch first --
 * the reported ones and the XA candidates -- and returns their number.  bmh_format_sam then takes, per record, its slot
 * in the bmh_cigar_batch outputs (slot[i], -1 = none) and returns the text (malloc'd; free with bmh_free), one line per
 * record in the reference's order, an unmapped record for reads without a reported alignment.  names: the read names,
 * NUL-terminated, back to back, name_off[r] the start of read r's.  Formats ranges of reads on host threads.  reads: nt4 codes (QUAL is '*':
 * bmh_format_sam_ex takes the qualities).  ALT contigs: po->contig_is_alt (soft clips on ALT hits, the pa:f tag, the XA limits); pairs: bmh_format_sam_pe. */
int64_t bmh_sam_need_cigar(const bmh_post_opt_t *po, const int32_t *fin, const uint32_t *fin_per_read, uint32_t n_reads, uint8_t *need);
char *bmh_format_sam(const bmh_post_opt_t *po, uint32_t n_reads, const char *names, const uint64_t *name_off, const uint8_t *reads,
                     const uint64_t *read_offs, const uint32_t *read_lens, int n_contigs, const char *const *contig_names,
                     const int64_t *contig_offset, const int32_t *fin, const uint32_t *fin_per_read, const int64_t *slot,
                     const int32_t *aln, const uint32_t *cigar, int max_cigar, const char *md, int md_cap, size_t *len_out);
void bmh_free(void *p);
/* bmh_format_sam with the read file's qualities and comments (FASTQ, -C): quals [.. same offsets as reads] Phred+33 or NULL (QUAL '*'); comments / comment_off
 * as names / name_off, or NULL (no comments).  QUAL covers SEQ's bases -- the hard clips of later records trimmed, reversed (not complemented) on the reverse
 * strand, '*' on 0x100 records (src/bwamem.c:1575-1612); with po->copy_comment a non-empty comment goes behind every record's tags (src/bwamem.c:1670-1673).
 * bmh_format_sam = bmh_format_sam_ex with NULLs; the same for pairs: bmh_format_sam_pe_ex. */
char *bmh_format_sam_ex(const bmh_post_opt_t *po, uint32_t n_reads, const char *names, const uint64_t *name_off, const uint8_t *reads,
                        const uint64_t *read_offs, const uint32_t *read_lens, const uint8_t *quals, const char *comments, const uint64_t *comment_off,
                        int n_contigs, const char *const *contig_names, const int64_t *contig_offset, const int32_t *fin, const uint32_t *fin_per_read,
                        const int64_t *slot, const int32_t *aln, const uint32_t *cigar, int max_cigar, const char *md, int md_cap, size_t *len_out);

/* bmh_format_sam_ex / bmh_format_sam_pe_ex (h_rec and unflag NULL: single-end reads) with a read group per read: the same table on the host -- read r's records
 * carry RG:Z:<ID read_group[r]>, ID g = ids[id_off[g] .. id_off[g + 1]), at the place po->rg_id's tag takes.  Refused: po->rg_id beside it, an index outside the table. */
typedef struct { const uint32_t *read_group; const char *ids; const uint32_t *id_off; uint32_t n_groups; } bmh_read_groups_t;
char *bmh_format_sam_groups(const bmh_post_opt_t *po, uint32_t n_reads, const char *names, const uint64_t *name_off, const uint8_t *reads,
                            const uint64_t *read_offs, const uint32_t *read_lens, const uint8_t *quals, const char *comments, const uint64_t *comment_off,
                            int n_contigs, const char *const *contig_names, const int64_t *contig_offset, const int32_t *fin, const uint32_t *fin_per_read,
                            const int32_t *h_rec, const int32_t *unflag, const int64_t *slot, const int32_t *aln, const uint32_t *cigar, int max_cigar,
                            const char *md, int md_cap, const bmh_read_groups_t *groups, size_t *len_out);

/* ---- the read file: one '>' header line and one sequence line per read, the only layout the reference's seeding library parses
 * (src/GPUSeed/seed_gen.cu:1698-1728; the host takes the same file through kseq, bseq_read src/bwa.c:48-66).  Loads it into the flat
 * arrays this API takes: the letters back to back (what bmh_seed_batch / bmh_chain_* read in HBM), their nt4 codes (nst_nt4_table,
 * src/bntseq.c: what the host tail and bmh_format_sam read), offsets, lengths, and the names (the header up to the first blank,
 * NUL-terminated, back to back: bmh_format_sam's names / name_off).  Blank lines are skipped, CR LF line ends accepted; headers and
 * sequence lines that do not alternate: BMH_EINVAL.  n_threads <= 0: all host threads.  Arrays are malloc'd: bmh_reads_free. */
/* FASTA or FASTQ (bmh_reads_load / bmh_reads_scan; the first non-blank byte decides, '>' or '@'): FASTQ records are four lines -- '@' header, ONE sequence
 * line, a '+' line, ONE quality line of the sequence's length --, blank lines between records and CR LF line ends accepted.  A quality line of another
 * length, a missing '+' line, a truncated last record, a record over more lines, FASTA and FASTQ records in one file: BMH_EINVAL with a message that
 * names it.  out->quals (FASTQ; NULL for FASTA): the qualities at the letters' offsets.  flags & BMH_READS_COMMENTS: out->comments / comment_offs /
 * n_comment_bytes hold every read's header comment (the text behind the first blank, as kseq cuts it: src/kseq.h:187, a trailing CR dropped at :140),
 * NUL-terminated back to back like the names ("" = none); else NULL / 0.  bmh_reads_load_fasta and bmh_fasta_scan take FASTA only, as before. */
#define BMH_READS_COMMENTS 1
/* bmh_fasta_scan: reads, bases, name bytes and the longest read of such a file -- out[4] -- from one counting pass of the mapped file, without loading it
 * (what a driver looks at before it chooses between bmh_aligner_run_fasta and the paths that take longer reads). */
int bmh_fasta_scan(const char *path, int n_threads, uint64_t *out);
int bmh_reads_scan(const char *path, int n_threads, uint64_t *out);
typedef struct {
	uint64_t n_reads, n_bases, n_name_bytes;
	uint8_t *ascii, *codes;        /* [n_bases] */
	uint64_t *offs;                /* [n_reads] start of read r in ascii / codes */
	uint32_t *lens;                /* [n_reads] */
	uint8_t *names;                /* [n_name_bytes] */
	uint64_t *name_offs;           /* [n_reads] */
	uint8_t *quals;                /* [n_bases] Phred+33 at the offsets of ascii, or NULL (no qualities: QUAL '*') */
	uint8_t *comments;             /* [n_comment_bytes] as names, or NULL (none) */
	uint64_t *comment_offs;        /* [n_reads] */
	uint64_t n_comment_bytes;
	uint32_t *groups;              /* [n_reads] every read's read group, an index into the run's table (BAM input that keeps its read groups), or NULL */
} bmh_read_set_t;
int bmh_reads_load_fasta(const char *path, int n_threads, bmh_read_set_t *out);
int bmh_reads_load(const char *path, int n_threads, int flags, bmh_read_set_t *out);
void bmh_reads_free(bmh_read_set_t *r);
/* One or two read files of any shape the reference takes (kseq_read / bseq_read, src/kseq.h:175-215, src/bwa.c:42-75): FASTA with sequences over any number
 * of lines, FASTQ (four-line, or with sequence and qualities over several lines), CR LF line ends, empty lines; plain, gzip (by the magic bytes; concatenated
 * members are one stream) or BGZF (inflated on n_threads host threads); regular files, pipes, process substitutions.  zlib is loaded at run time
 * (libz.so.1); without it a gzip file is refused with a message.  path2 (or NULL): the mates -- read i of path1 and read i of path2 become reads 2i and
 * 2i+1, both names without a trailing "/<digit>"; the two files hold the same kind of records.  The records are cut on the device (csrc/reads_parse.hip);
 * text it cannot decide (multi-line FASTQ, stray '+' / '@' lines, text before the first header) is walked by the host.  flags: BMH_READS_COMMENTS as above;
 * BMH_READS_HOST: the host walker alone (no device needed).  Refused with a message (BMH_EINVAL): a truncated or damaged gzip stream, qualities of another
 * length than the sequence, a truncated last record, an empty sequence, FASTA and FASTQ records mixed (in one file or between the two), a pair whose two
 * names differ, a file that ends before the other -- in that last case *out holds the complete pairs before the end (free it as usual).
 */
#define BMH_READS_HOST 2
int bmh_reads_load_files(const char *path1, const char *path2, int n_threads, int flags, bmh_read_set_t *out);
/* ---- BAM as read input (csrc/bam_in_core.h, csrc/bam_in_kernels.hip): unaligned BAM, or an aligned one grouped by read name.  bmh_reads_load_files and
 * bmh_aligner_run_files take a BGZF file whose inflated bytes begin with "BAM\1" -- recognised from those bytes, a regular file or a pipe -- in place of a text file;
 * a mates file beside it and a BAM in a plain gzip stream are refused with a message.  The rules are those of `samtools fastq`: records with flag 0x100 or 0x800
 * give no read; a record with flag 0x10 gives its read back in sequencing orientation (bases complemented and reversed, qualities reversed); letters from
 * "=ACMGRSVTWYHKDBN"; qualities + 33, a record whose qualities are all 0xff has none (quals is NULL when no record has any; a file that mixes both, a quality above
 * 93 and l_seq 0 are refused); names verbatim.  Flag 0x1 on the first record kept means pairs: the two records of a pair are adjacent, in either order, and the 0x40
 * record becomes read 2i, the 0x80 record read 2i+1 (two names, two records of one role, a record without partner, 0x1 on some records only: refused, naming the
 * record's index in the file).  With BMH_READS_COMMENTS the tags become the comment: XX:T:value fields joined by tabs in file order, A as it is, c C s S i I as i,
 * Z and H copied; f and B tags are left out, and so are NM MD AS XS SA XA pa RG MC MQ.  The header's text and reference table, refID, pos, mapq, the CIGAR and the
 * mate fields are ignored.  The host walks the chain of record starts (a record names its own length) over each inflated window -- BAM therefore always takes the
 * host inflate, also with BMH_INFLATE_DEVICE=1 --; validation, pairing, the scans, bases, qualities, names and comments are kernels.  A record that fails a check
 * hands its window to the host form, which words the refusal.
 * bmh_bam_reads_device / bmh_bam_reads_host: the step on its own -- uncompressed BAM records in host memory, without the header, as one read set (bmh_reads_free);
 * flags: BMH_READS_COMMENTS.  bmh_reads_last_bam_counts: out[2] of the process's last such call, bmh_reads_load_files or bmh_aligner_run_files call: records
 * skipped (0x100 / 0x800), f and B tags left out.
 * bmh_aligner_set_bam_pairs: bmh_aligner_run_files is told `paired` before it has opened its file; when a BAM then turns out to hold pairs and paired was 0, the
 * run takes this batch_bases (0: the argument's; ignored with batch_reads) and this n_lanes (0: the argument's) in place of its arguments.  A BAM without flag 0x1
 * and paired != 0 is refused. */
int bmh_bam_reads_device(const uint8_t *records, uint64_t n_bytes, int flags, bmh_read_set_t *out);
int bmh_bam_reads_host(const uint8_t *records, uint64_t n_bytes, int flags, bmh_read_set_t *out);
/* The same step for a run that keeps the input's read groups: rg_ids [n_groups] are the IDs of the header's @RG lines (1 .. 255 bytes each, no two equal), and
 * out->groups [n_reads] is the index of every read's RG:Z value among them -- whole IDs compared.  Refused naming the record's index: a kept record without an RG
 * tag, with one of another type than Z or with an ID that is not listed, a pair whose two records name different groups.  Records skipped by their flag are not looked at.
 * bmh_bam_header_read_groups: the @RG lines of a BAM header's text (it ends at its first NUL; CR LF accepted; the last line may lack its newline; other lines
 * ignored) -- *lines: the lines verbatim, each with a '\n' behind it; *lib [*n_groups]: every group's library by first appearance (the last non-empty LB field;
 * groups without one share a library); bmh_free both.  Refused naming the line: no @RG line, a line without a non-empty ID of at most 255 bytes or with a field that
 * is not XX:value, a repeated ID, more than 65535 groups, and with markdup != 0 more than 255 libraries. */
int bmh_bam_reads_groups_device(const uint8_t *records, uint64_t n_bytes, int flags, const char *const *rg_ids, int n_groups, bmh_read_set_t *out);
int bmh_bam_reads_groups_host(const uint8_t *records, uint64_t n_bytes, int flags, const char *const *rg_ids, int n_groups, bmh_read_set_t *out);
int bmh_bam_header_read_groups(const char *text, uint64_t n_bytes, int markdup, char **lines, uint64_t *lines_bytes, int32_t **lib, int32_t *n_groups);
int bmh_reads_last_bam_counts(uint64_t *out);
/* ---- Mates collated by name (--collate; csrc/bam_collate_core.h has the definition): a paired BAM in any record order -- a coordinate-sorted one, the aligner's
 * own --sort output among them -- is taken as read input.  Off by default, and with it off every path is what it was.  Kept records (no flag 0x100 / 0x800) are
 * taken in file order, numbered as the messages number them, and every check made on a kept record still applies.  A record whose name (all its bytes up to the
 * NUL) is open closes that record: the two are a pair, the 0x40 record read 2k and the 0x80 record read 2k+1, completed at the later record; two records of one
 * role under one open name are refused, naming both.  Any other record opens its name.  The reads are the pairs in the order of their completion and batches are
 * cut over that sequence by the usual rule, so the read set, the cuts and the SAM depend on the file and the batch size alone -- never on the windows -- and equal
 * those of a run without the option on the name-grouped BAM that holds the same pairs in that order.  Records skipped by their flag open and close nothing.  At
 * the file's end, after every complete batch, an open record is refused ("flag 0x1 and no partner", the smallest index named; bmh_reads_load_files and
 * bmh_bam_reads_* then leave the complete pairs in *out).  With the input's read groups kept, a pair of two groups is refused naming both records.  A single-end
 * BAM gives what it gives without the option; text input is refused.
 * A window is consumed up to the record that completes the last pair of its batch; the open records inside that prefix move into a pool in host memory (their
 * bytes, each with its file index), which the host form and the device form share.  The device keeps the pool's keys only (name hash, role, slot): per window it
 * hashes the kept records' names (64-bit FNV-1a), sorts them with the pool's keys (rocPRIM), matches runs of equal hashes (names compared byte by byte), ranks the
 * pairs by a scan over the completions, and hands the prefix's open records back as an index list; a pool record that a window record closes is copied behind the
 * window's bytes by the host and decoded like any other record, so the extended window stays below 2^31 bytes.  A run of equal hashes that is not one 0x40 and one
 * 0x80 record of one name hands the window to the host form (counted: windows_to_host_for_hash_runs).  The knob COLLATE_HASH_BITS (bmh_tune_set; default 64) cuts
 * the hash to its low bits, for tests that force equal hashes.
 * The open records' bytes (4 + block_size each) are capped: mem_bytes, 0 for the default of 8 GiB.  They are held against the cap at every completion; beyond it
 * the run stops after the batches before it have been written, naming the option, the cap and the record.  Nothing is spilled to disk.  The 2^31-byte limit on one
 * window stays: a file in which one batch's pairs complete only across more than 2^31 bytes of records is refused.
 * The cap counts the records' bytes alone: the pool's bookkeeping (a slot, a vector and a name key per open record, on the order of 150 bytes) comes on top.
 * bmh_reads_load_files_ex / bmh_bam_reads_ex: the readers with every option -- collate_mem is that cap (0: the default; refused without BMH_READS_COLLATE);
 * bmh_bam_reads_ex takes BMH_READS_HOST for the host form and rg_ids (or NULL) as bmh_bam_reads_groups_* take them.  BMH_READS_KEEP_RG: bmh_reads_load_files reads
 * a BAM under its own read groups as bmh_aligner_set_keep_rg does -- the header's @RG lines are the table, out->groups [n_reads] the index of every read's line.
 * BMH_READS_COLLATE: the flag bit of bmh_reads_load_files, bmh_bam_reads_device / _host and their _groups forms.  bmh_aligner_set_collate: for bmh_aligner_run_files
 * (text input is then refused) and every group of bmh_aligner_run_groups whose input is a BAM; mem_bytes without `on` is refused.  bmh_reads_last_collate_counts:
 * of the process's last such call -- pairs, those whose two records were adjacent, the peaks of the open records and their bytes, windows handed to the host form
 * for a run of equal hashes. */
#define BMH_READS_COLLATE 4
#define BMH_READS_KEEP_RG 8
int bmh_reads_load_files_ex(const char *path1, const char *path2, int n_threads, int flags, uint64_t collate_mem, bmh_read_set_t *out);
int bmh_bam_reads_ex(const uint8_t *records, uint64_t n_bytes, int flags, const char *const *rg_ids, int n_groups, uint64_t collate_mem, bmh_read_set_t *out);
typedef struct { uint64_t pairs, pairs_adjacent, open_records_peak, open_bytes_peak, windows_to_host_for_hash_runs; } bmh_collate_counts_t;
int bmh_reads_last_collate_counts(bmh_collate_counts_t *out);

/* ---- BGZF members inflated on the device (csrc/inflate_core.h, csrc/inflate_kernels.hip): all of RFC 1951, one lane per member, the CRC32 of the text
 * computed and compared there too.  BGZF (what bgzip writes) is a series of gzip members of at most 64 KiB of text, each naming its own size in the extra
 * field "BC" and its text's size and CRC32 in its trailer; a plain gzip stream is one dependent bit stream and is not taken here.
 * bmh_bgzf_scan (host only): the whole members at the front of data[0 .. n_bytes) as table entries -- tab may be NULL to count; at most tab_cap are
 * written.  *used: the bytes they cover (less than n_bytes: the next member's header or body is cut, or tab_cap was reached); *text_bytes: the sum of
 * their ISIZE; out_off is the prefix sum of ISIZE, so every member's text lands at its final place.  BMH_EINVAL: bytes that begin no BGZF member.
 * bmh_inflate_members_device: n members on `stream` -- d_in [in_bytes] the compressed bytes, d_tab [n], d_out [out_bytes] the text, d_status [n] one
 * word per member: 0, or the check that failed (bmh_inflate_status_name says which: block type 3, LEN / NLEN, a bad code-length set, no such symbol,
 * a distance beyond the text, data that end early, a size other than ISIZE, the CRC32, a table entry outside the buffers).  A damaged member cannot
 * make the kernel read or write outside the member's own bytes and text.  bmh_inflate_members_host: the same decoder as plain C++ on host threads.
 * bmh_bgzf_inflate: the text of a whole BGZF file held in host memory (malloc'd, NUL behind it; free with bmh_free); flags: BMH_INFLATE_HOST runs
 * the host decoder (no device needed).  Refused with a message: a cut file, bytes that are no BGZF member, a damaged member (named by its index). */
typedef struct {
	uint64_t in_off;       /* where the member's deflate data begin in the compressed buffer */
	uint64_t out_off;      /* where its text goes in the output */
	uint32_t in_len;       /* bytes of deflate data */
	uint32_t isize;        /* bytes of text (the trailer's ISIZE; at most 65536) */
	uint32_t crc32;        /* of the text (the trailer's) */
	uint32_t reserved;
} bmh_inflate_member_t;
#define BMH_INFLATE_HOST 1
int bmh_bgzf_scan(const uint8_t *data, uint64_t n_bytes, bmh_inflate_member_t *tab, uint64_t tab_cap, uint64_t *n_members, uint64_t *used, uint64_t *text_bytes);
int bmh_inflate_members_device(const uint8_t *d_in, uint64_t in_bytes, const bmh_inflate_member_t *d_tab, uint32_t n, uint8_t *d_out, uint64_t out_bytes,
                               uint32_t *d_status, void *stream);
int bmh_inflate_members_host(const uint8_t *in, uint64_t in_bytes, const bmh_inflate_member_t *tab, uint32_t n, uint8_t *out, uint64_t out_bytes,
                             uint32_t *status, int n_threads);
const char *bmh_inflate_status_name(uint32_t status);
int bmh_bgzf_inflate(const uint8_t *data, uint64_t n_bytes, int flags, uint8_t **text, uint64_t *text_bytes);

/* ---- interleaved pairs (read 2i, 2i+1): mem_pestat, mem_matesw (mate rescue, host local alignment), mem_pair, mem_sam_pe
 * (src/bwamem_pair.c).  Same inputs as bmh_finalize_regs plus read_lens and contig_len; out has room for `cap` records
 * (mate rescue adds regions: regions_in + 16 per read is ample).  out_h[r]: the record of read r's own alignment within
 * its list (-1 unmapped); out_unflag[r]: pair flags of the unmapped record of a read without reported alignment;
 * pes_out[4][5] (optional) = {low, high, failed, avg, std} per orientation FF, FR, RF, RR.  popt->id0 = index of the
 * batch's first READ in the run.  The insert-size statistics are those of the batch, as in the reference. */
typedef struct { int pen_unpaired, max_ins, max_matesw; int no_rescue, no_pairing; } bmh_pe_opt_t;       /* 17, 10000, 50; -S, -P */
void bmh_pe_opt_default(bmh_pe_opt_t *o);
int64_t bmh_finalize_pairs(const bmh_chain_opt_t *copt, const bmh_ext_params_t *ep, const bmh_post_opt_t *popt, const bmh_pe_opt_t *pe,
                           int64_t l_pac, const uint8_t *pac, uint32_t n_reads, const uint8_t *reads, const uint64_t *read_offs,
                           const uint32_t *read_lens, const int32_t *regs_in, const uint32_t *regs_per_read, const float *frac_rep,
                           int n_contigs, const int64_t *contig_offset, const int32_t *contig_len,
                           int32_t *out, uint64_t cap, uint32_t *out_per_read, int32_t *out_h, int32_t *out_unflag, double *pes_out,
                           int n_threads);
/* bmh_finalize_pairs with the local alignments of the mate rescue (mem_matesw's ksw_align2 calls, 98 % of its time on a repeat-rich
 * batch) computed as ONE batch on the device (csrc/pair_kernels.hip: the striped kernel's lanes as GPU lanes).  idx: the index with
 * its 2-bit reference in HBM; d_reads / d_offs: the batch's ASCII reads in HBM (the same reads as `reads`); stream: waited for.
 * Same results as bmh_finalize_pairs, record for record. */
int64_t bmh_finalize_pairs_dev(const bmh_index_t *idx, const uint8_t *d_reads, const uint32_t *d_offs, void *stream,
                               const bmh_chain_opt_t *copt, const bmh_ext_params_t *ep, const bmh_post_opt_t *popt, const bmh_pe_opt_t *pe,
                               int64_t l_pac, const uint8_t *pac, uint32_t n_reads, const uint8_t *reads, const uint64_t *read_offs,
                               const uint32_t *read_lens, const int32_t *regs_in, const uint32_t *regs_per_read, const float *frac_rep,
                               int n_contigs, const int64_t *contig_offset, const int32_t *contig_len,
                               int32_t *out, uint64_t cap, uint32_t *out_per_read, int32_t *out_h, int32_t *out_unflag, double *pes_out,
                               int n_threads);
/* mem_sort_dedup_patch alone on the device (csrc/regs_kernels.hip: the first step of bmh_finalize_regs_device, the step the tail of interleaved
 * pairs shares with it): arguments as bmh_finalize_regs_device without d_frac_rep; d_out [n_regs][16] receives, grouped by read in the input's
 * order, the regions that are left -- [0] read, [1] score, [2] qb, [3] qe, [4..7] rb / re, [8] truesc, [9] w (a patched region carries a wider
 * band), [13] its sequence; the other fields are unspecified --, d_out_per_read their numbers.  Returns their total or a negative BMH_E* code
 * (BMH_ECAPACITY: a read beyond the kernels' fixed limits: the caller takes the host form); waits for the stream.  ALT tables are not looked at.
 * bmh_finalize_pairs_deduped: bmh_finalize_pairs_dev from those records (copied to the host) instead of the regions: same results. */
int64_t bmh_dedup_regs_device(const bmh_index_t *idx, const bmh_chain_opt_t *copt, const bmh_ext_params_t *ep, const bmh_post_opt_t *popt,
                              const uint8_t *d_reads, const uint32_t *d_offs, uint32_t n_reads,
                              const int32_t *d_regs, uint64_t n_regs, const uint32_t *d_regs_per_read,
                              int n_contigs, const int64_t *contig_offset, int32_t *d_out, uint32_t *d_out_per_read, void *stream);
int64_t bmh_finalize_pairs_deduped(const bmh_index_t *idx, const uint8_t *d_reads, const uint32_t *d_offs, void *stream,
                                   const bmh_chain_opt_t *copt, const bmh_ext_params_t *ep, const bmh_post_opt_t *popt, const bmh_pe_opt_t *pe,
                                   int64_t l_pac, const uint8_t *pac, uint32_t n_reads, const uint8_t *reads, const uint64_t *read_offs,
                                   const uint32_t *read_lens, const int32_t *dedup_recs, const uint32_t *dedup_per_read, const float *frac_rep,
                                   int n_contigs, const int64_t *contig_offset, const int32_t *contig_len,
                                   int32_t *out, uint64_t cap, uint32_t *out_per_read, int32_t *out_h, int32_t *out_unflag, double *pes_out,
                                   int n_threads);
/* The windows of the mate rescue (mem_matesw up to its ksw_align2 call, src/bwamem_pair.c:119-150) are found by the host's walk of every pair; with the knob
 * ALIGNER_RESCUE_DEV=1 bmh_aligner_run finds them with a kernel on the regions the device keeps (csrc/pair_kernels.hip: rescue_jobs_kernel; same records,
 * measured slower on a busy device).  With the knob RESCUE_CHECK set as well the host's walk runs beside the kernel; out[5] = batches checked, pairs,
 * alignments the device asked for, pairs whose "a call reached a window" flag differs (0: the flag decides which pairs the host walks), pairs whose list of
 * calls differs (the host walk's mem_sort_dedup_patch calls can change a list; such a call is then computed by the host's second walk). */
void bmh_rescue_check_counts(uint64_t *out);
int64_t bmh_sam_need_cigar_pe(const bmh_post_opt_t *po, const int32_t *fin, const uint32_t *fin_per_read, const int32_t *h_rec,
                              uint32_t n_reads, uint8_t *need);
char *bmh_format_sam_pe(const bmh_post_opt_t *po, uint32_t n_reads, const char *names, const uint64_t *name_off, const uint8_t *reads,
                        const uint64_t *read_offs, const uint32_t *read_lens, int n_contigs, const char *const *contig_names,
                        const int64_t *contig_offset, const int32_t *fin, const uint32_t *fin_per_read, const int32_t *h_rec,
                        const int32_t *unflag, const int64_t *slot, const int32_t *aln, const uint32_t *cigar, int max_cigar,
                        const char *md, int md_cap, size_t *len_out);
char *bmh_format_sam_pe_ex(const bmh_post_opt_t *po, uint32_t n_reads, const char *names, const uint64_t *name_off, const uint8_t *reads,
                           const uint64_t *read_offs, const uint32_t *read_lens, const uint8_t *quals, const char *comments, const uint64_t *comment_off,
                           int n_contigs, const char *const *contig_names, const int64_t *contig_offset, const int32_t *fin, const uint32_t *fin_per_read,
                           const int32_t *h_rec, const int32_t *unflag, const int64_t *slot, const int32_t *aln, const uint32_t *cigar, int max_cigar,
                           const char *md, int md_cap, size_t *len_out);

/* ------------------------------------------------- device job builder (SURVEY 8f ranks 1-2 on the GPU) */

/* The same stage as bmh_build_jobs, on the device: seeds of bmh_seed_batch (still in HBM) -> chains -> filtered
 * chains -> regions and their LEFT/RIGHT extension jobs, with the query bases taken from the reads and the target
 * bases fetched from the index's 2-bit reference on the device (bns_fetch_seq, src/bntseq.c:531-580, and the
 * LEFT-side reversal of src/bwamem.c:1328-1334).  The batch is byte-identical to bmh_build_jobs' and feeds
 * bmh_extend_batch directly; bmh_chain_merge then turns the extension results into regions.
 * The index must have been uploaded with its pac. */
typedef struct bmh_chain_ws bmh_chain_ws_t;
bmh_chain_ws_t *bmh_chain_ws_create(uint32_t max_reads, uint64_t max_seeds);
void bmh_chain_ws_free(bmh_chain_ws_t *ws);
/* contig table of the reference (host arrays, as in bmh_build_jobs); default: one sequence of l_pac bases */
int bmh_chain_set_contigs(bmh_chain_ws_t *ws, int n_contigs, const int64_t *contig_offset, const int32_t *contig_len);
/* which of them are ALT contigs (is_alt[n_contigs], host memory; NULL or all zero: none) -- call after bmh_chain_set_contigs */
int bmh_chain_set_alt(bmh_chain_ws_t *ws, int n_contigs, const uint8_t *is_alt);
/* The extension cap of the workspace: bmh_chain_extend and bmh_chain_extend_merge send query sides of 769 .. cap bases to the long-query
 * classes of bmh_extend_batch_long.  Default (and any cap up to 768): the classes of bmh_extend_batch alone.  A batch with a longer query
 * side makes either call return BMH_EINVAL with a message that names the cap, and no region of it comes back.  Reads of up to
 * BMH_EXT_LONG_MAX bases are chained (those beyond 700 one wave per read, in wide records); a longer read makes the chaining call
 * return BMH_EINVAL.  cap > BMH_EXT_LONG_MAX: BMH_EINVAL. */
int bmh_chain_ws_set_max_qlen(bmh_chain_ws_t *ws, uint32_t cap);

typedef struct {
	uint64_t n_jobs, n_regs, q_bytes, t_bytes;
	uint64_t n_heavy_reads;          /* reads chained by a whole wave (more than BMH_CHAIN_HEAVY=16 sampled seed occurrences) */
	const uint8_t *d_q; const uint32_t *d_qoff, *d_qlen;          /* the bmh_extend_batch inputs */
	const uint8_t *d_t; const uint32_t *d_toff, *d_tlen, *d_h0;
	const uint32_t *d_job_read, *d_job_reg, *d_job_side;           /* read / region / side (0 left, 1 right) per job */
	const uint32_t *d_regs_per_read;                               /* [n_reads] */
	const float *d_frac_rep;                                       /* [n_reads] frac_rep of the read's chains (for bmh_finalize_regs) */
} bmh_dev_jobs_t;

/* kernel times of the last bmh_chain_batch / bmh_chain_extend_merge in ms (HIP events): [0] classify [1] lane kernel (reads that
 * sample at most 16 seed occurrences) [2] wave kernels (the others, one wave per read, size classes by LDS scratch of 64 ... 1250
 * entries on side streams) [3] the stage up to the (first) counts; [6] reads whose scratch has at most 512 entries, [7] the larger ones */
void bmh_chain_last_timing(const bmh_chain_ws_t *ws, float ms[8]);

/* which form chained how many reads of the last bmh_chain_batch / bmh_chain_extend_merge: out[0..11) reads per size class of the cooperative
 * kernels (at most 16, 32, 64, 128, 256, 384, 512, 620, 1250, 1860 sampled seed occurrences, more), out[11..15) reads per bin of the lane
 * kernel (at most 2, 4, 8 occurrences, the rest up to BMH_CHAIN_HEAVY), out[15] reads beyond 700 bases (chained by their own kernel) */
int bmh_chain_class_counts(const bmh_chain_ws_t *ws, uint32_t out[16]);

/* on (default): bmh_chain_batch also materialises the base arrays d_q/d_t/d_qoff/d_toff for bmh_extend_batch;
 * off: it stops at the job descriptors (those four pointers come back NULL, q_bytes = t_bytes = 0) and the batch is
 * extended with bmh_chain_extend, which reads the bases where they already are (reads, 2-bit reference). */
int bmh_chain_set_materialize(bmh_chain_ws_t *ws, int on);

/* d_reads/d_offs/d_lens: as for bmh_seed_batch; seeds: its output for the same reads.  Pointers in *out stay valid
 * until the next call on the workspace.  Synchronises the stream (once for the region/job counts, once more for the
 * base counts when materialising). */
int bmh_chain_batch(bmh_chain_ws_t *ws, const bmh_chain_opt_t *opt, const bmh_index_t *idx, const uint8_t *d_reads,
                    const uint32_t *d_offs, const uint32_t *d_lens, uint32_t n_reads, const bmh_seeds_t *seeds,
                    void *stream, bmh_dev_jobs_t *out);
/* bmh_extend_batch on the jobs of the last bmh_chain_batch, without materialised base arrays: same results (d_out3
 * [n_jobs][3], optional d_raw [n_jobs][6]).  d_reads and the index of that call must still be alive.  Asynchronous. */
int bmh_chain_extend(bmh_chain_ws_t *ws, const bmh_ext_params_t *p, int32_t *d_out3, int32_t *d_raw, void *stream);
/* d_out3 = extension results of the batch's jobs -> d_regs_out[n_regs][8] =
 * {read, score, qb, qe, rb_lo, rb_hi, re_lo, re_hi} (src/bwamem.c:2297-2303).  Asynchronous on stream. */
int bmh_chain_merge(bmh_chain_ws_t *ws, const int32_t *d_out3, int32_t *d_regs_out, void *stream);

/* bmh_chain_batch + bmh_chain_extend + bmh_chain_merge in ONE call that hides the chaining of the seed-rich reads behind the
 * extension of the others (two passes: the reads that sample at most 16 seed occurrences are chained, turned into jobs and
 * extended while one wave per read is still chaining the rest on side streams; then the rest).  d_regs_out [cap_regs_out][8]
 * receives the regions in read order -- the same array the three-call form produces; out->n_regs / n_jobs / d_regs_per_read /
 * d_frac_rep as for bmh_chain_batch; the job arrays in *out are in pass order (all jobs of the first pass, then the second);
 * d_q / d_t are not materialised.  Synchronises the stream twice (counts); the second extension and the merge are still in
 * flight on `stream` when it returns.  The short kernels the first extension pass waits for (classification, the lane kernel, the
 * counts) run on a stream of the highest priority owned by the workspace, behind a host-side wait for `stream` (see bmh_seed_batch;
 * BMH_CHAIN_LIGHT_PRIO=normal when the workspace is created: on `stream`); the wave-per-read classes on streams of the lowest.  BMH_ECAPACITY if the batch has more than cap_regs_out regions. */
int bmh_chain_extend_merge(bmh_chain_ws_t *ws, const bmh_chain_opt_t *opt, const bmh_index_t *idx, const uint8_t *d_reads,
                           const uint32_t *d_offs, const uint32_t *d_lens, uint32_t n_reads, const bmh_seeds_t *seeds,
                           const bmh_ext_params_t *ep, int32_t *d_regs_out, uint64_t cap_regs_out, void *stream, bmh_dev_jobs_t *out);
/* of the last bmh_chain_extend_merge (waits for it): ms[0], ms[1] = extension of the two passes, ms[2] = the whole call's device
 * time; jobs[0], jobs[1] = extension jobs of the two passes */
int bmh_chain_extend_merge_timing(const bmh_chain_ws_t *ws, float ms[3], uint64_t jobs[2]);

/* ------------------------------------------------- region -> CIGAR / NM / MD */

/* mem_reg2aln (src/bwamem.c:2344-2440) for n regions: banded global alignment ksw_global2 (src/ksw.c:1120-1241) of
 * read[qb,qe) against the reference text [rb,re) with the band of bwa_gen_cigar2 (src/bwa.c:111-216), the retry with a
 * doubled band, NM, the MD string, the squeeze of a leading / trailing deletion, soft clips and the position.
 * d_regs: records of reg_stride int32: 8 = {read, score, qb, qe, rb_lo, rb_hi, re_lo, re_hi}, the layout bmh_chain_merge /
 * bmh_merge_regs write (truesc = score, region band = opt_w); 16 = the records of bmh_finalize_regs (truesc and the
 * region's band at [8], [9]: a patched region carries a wider band).  d_sel (optional): n indices into d_regs, NULL = the
 * first n regions.  opt_w = mem_opt_t.w (300).
 * Out, per job: d_cigar[max_cigar] (len << 4 | op, op 0 M, 1 I, 2 D, 3 S), d_aln[8] = {pos_lo, pos_hi (0-based,
 * forward strand of the concatenated reference), is_rev, n_cigar, NM, global score, MD length, flags (1 = more than
 * max_cigar-2 ops, 2 = interval rejected by bwa_gen_cigar2, 4 = too large: a side of 2^20 bases or more, or a region beyond 704
 * bases whose band -- max(4 opt_w, |rlen - qlen| + 3) -- needs a direction matrix (min(qlen, 2 band + 1) x rlen bytes) over 1 GiB, never
 * the case for sides up to 32 768 bases; 8 = MD longer than md_cap -- reported where the operations fit: with flag 1 NM and MD
 * follow the operations that were kept and mean nothing, the caller redoes the job with larger slots)}, d_md[md_cap]
 * (NUL-terminated; d_md may be NULL).  The index must carry its pac.  Synchronises the stream once (sizes). */
int bmh_cigar_batch(const bmh_index_t *idx, const uint8_t *d_reads, const uint32_t *d_offs, const uint32_t *d_lens,
                    const int32_t *d_regs, int reg_stride, const uint32_t *d_sel, uint32_t n, const bmh_ext_params_t *p, int opt_w,
                    int max_cigar, uint32_t *d_cigar, int32_t *d_aln, int md_cap, char *d_md, void *stream);

/* frees the (device, stream) scratch of bmh_cigar_batch (device buffers it keeps between calls: the direction matrices of a batch are gigabytes);
 * the stream idle, its device current -- bmh_extend_release(stream) calls it too */
void bmh_cigar_release(void *stream);

/* ---- what the SAM writer needs of a batch, chosen and packed on the device (csrc/sam_kernels.hip)
 * bmh_sam_select_device: bmh_sam_need_cigar over records in HBM (d_fin [m][16], d_fin_per_read [n_reads]: what bmh_finalize_regs_device
 * left; d_h_rec: NULL, or for interleaved pairs the own-alignment record of every read as in bmh_sam_need_cigar_pe).  d_sel [m]
 * receives the indices of the selected records in ascending order -- the d_sel of bmh_cigar_batch --, d_slot [m] the place of every
 * record in that list or -1 (the slot[] of bmh_format_sam, 32-bit).  d_work: bmh_sam_select_work(n_reads, m) bytes of device memory.
 * Returns the number selected (waits for the stream) or a negative BMH_E* code.
 * bmh_cigar_pack_sizes / bmh_cigar_pack: the outputs of bmh_cigar_batch without their padding.  _sizes fills d_off [n + 1] with the
 * start (in 32-bit words) of every alignment in the packed array and returns the total number of words (waits for the stream):
 * n_cigar operations, then -- with_md -- the MD string with its NUL, padded to a word; an alignment flagged 1, 4 or 8 takes no words
 * (the caller redoes it with larger slots).  bmh_cigar_pack then copies (asynchronous; md_cap a multiple of 4; d_md NULL if _sizes
 * was called with with_md = 0).  d_work: bmh_cigar_pack_work(n) bytes. */
size_t bmh_sam_select_work(uint32_t n_reads, uint64_t m);
int64_t bmh_sam_select_device(const bmh_post_opt_t *popt, const int32_t *d_fin, const uint32_t *d_fin_per_read, const int32_t *d_h_rec,
                              uint32_t n_reads, uint64_t m, uint32_t *d_sel, int32_t *d_slot, void *d_work, size_t work_bytes, void *stream);
size_t bmh_cigar_pack_work(uint32_t n);
int64_t bmh_cigar_pack_sizes(const int32_t *d_aln, uint32_t n, int with_md, uint32_t *d_off, void *d_work, size_t work_bytes, void *stream);
int bmh_cigar_pack(const int32_t *d_aln, const uint32_t *d_cigar, int max_cigar, const char *d_md, int md_cap, uint32_t n,
                   const uint32_t *d_off, uint32_t *d_packed, void *stream);

/* ---- the SAM text itself written on the device (csrc/sam_kernels.hip): the text of bmh_format_sam / bmh_format_sam_pe, byte for byte,
 * from records, alignments and packed CIGARs that never leave HBM.  Every pointer of bmh_sam_dev_t is device memory.  ALT contigs: with
 * popt->contig_is_alt set the records are ALT-mode records (bmh_post_opt_t: [11] the XA tag's key, [15] carries is_alt and alt_sc) and the
 * text follows (soft clips on ALT hits, the larger XA limit, pa:f written as printf's %.3f).
 * bmh_sam_text_sizes: first pass, d_text_off [n_reads + 1] = start of every read's records in the text; returns the text's length
 * (waits for the stream).  bmh_sam_text_write: second pass into d_text (asynchronous; the same d_work, untouched in between);
 * d_quals / d_comments + d_comment_off: as bmh_format_sam_ex's quals / comments / comment_off (d_comment_off [n_reads + 1]), NULL = none;
 * bmh_sam_text_check afterwards waits for the stream and reports an inconsistency between the passes.  d_work: bmh_sam_text_work bytes. */
typedef struct {
	uint32_t n_reads;
	const char *d_names; const uint64_t *d_name_off;           /* names NUL-terminated back to back; [n_reads + 1]: start of read r's, [n_reads] = their total length */
	const uint8_t *d_reads; const uint32_t *d_offs, *d_lens;   /* the batch's ASCII reads (what bmh_seed_batch takes) */
	int n_contigs; const char *d_contig_names; const uint32_t *d_contig_name_off; const int64_t *d_contig_offset;   /* names as above, [n_contigs + 1] */
	const int32_t *d_fin; const uint32_t *d_fin_per_read;      /* records [m][16], records per read */
	const int32_t *d_slot;                                     /* [m] record -> alignment (bmh_sam_select_device) */
	const int32_t *d_aln; const uint32_t *d_cig_off, *d_packed; /* bmh_cigar_batch's d_aln; bmh_cigar_pack's d_off / d_packed (with MD) */
	const int32_t *d_h_rec, *d_unflag;                         /* interleaved pairs (bmh_finalize_pairs' out_h / out_unflag) or NULL */
	const uint8_t *d_quals;                                    /* Phred+33 at d_offs, or NULL (QUAL '*') */
	const char *d_comments; const uint64_t *d_comment_off;     /* as d_names / d_name_off, or NULL (written only with popt->copy_comment) */
	/* per-read read groups, or NULL / 0 (popt->rg_id on every record, as before): read r's records carry RG:Z:<ID d_read_group[r]> where popt->rg_id's tag goes;
	 * the IDs lie back to back without terminators, ID g = d_rg_ids[d_rg_id_off[g] .. d_rg_id_off[g + 1]) (d_rg_id_off [n_rg + 1]).  Not beside popt->rg_id. */
	const uint32_t *d_read_group; const char *d_rg_ids; const uint32_t *d_rg_id_off; uint32_t n_rg;
} bmh_sam_dev_t;
size_t bmh_sam_text_work(uint32_t n_reads);
int64_t bmh_sam_text_sizes(const bmh_post_opt_t *popt, const bmh_sam_dev_t *d, uint64_t *d_text_off, void *d_work, size_t work_bytes, void *stream);
int bmh_sam_text_write(const bmh_post_opt_t *popt, const bmh_sam_dev_t *d, const uint64_t *d_text_off, char *d_text, void *d_work, size_t work_bytes, void *stream);
int bmh_sam_text_check(const void *d_work, uint32_t n_reads, void *stream);

/* ------------------------------------------------- reads in host memory -> SAM text, batches driven by C threads (csrc/align_pipeline.hip)
 *
 * What gase_aln's worker threads do around the device libraries (src/bwamem.c:2042-2340, src/fastmap.c:59-120), on top of the entry
 * points above: n_lanes worker threads take the batches [cuts[b], cuts[b+1]) of the read set in turn -- each with its own stream,
 * workspaces and pinned staging: H2D, seeding, chaining, extension, merge, the region tail, the selection of the records that need a
 * CIGAR, CIGAR / NM / MD, and the SAM text itself (bmh_sam_text_*), all on the device; the text goes to the host -- and ONE writer
 * thread hands every batch's text to `sink` in order (return 0 to go on) while the workers are on the next ones.  Interleaved pairs:
 * mem_sort_dedup_patch, mem_mark_primary_se and, for the pairs the mate rescue does not touch, mem_pair and mem_sam_pe's choices on
 * the device too; the insert-size statistics, the rescue's bookkeeping and the pairs it touches on n_threads host threads in the
 * middle of the batch.  An index with ALT contigs: the same (the device tail and the pairing kernel know the ALT rules).  A batch the device tail refuses (BMH_ECAPACITY)
 * takes the host tail.  The text is what
 * bmh_format_sam / bmh_format_sam_pe write, byte for byte (records only: the caller writes the @SQ header).  A read set with quals (FASTQ) gets QUAL,
 * one with comments and popt->copy_comment the comments (bmh_format_sam_ex): they go to the device beside the letters and names; without them nothing more is sent.
 * cuts: n_batches + 1 read indices, cuts[0] = 0, cuts[n_batches] = n_reads, even batch sizes when paired (the reference cuts its
 * batches by bases, bseq_read src/bwa.c:48-66, and the insert-size statistics are those of a batch).  popt->id0 is ignored (a batch's
 * id0 is its first read).  Reads of up to BMH_EXT_LONG_MAX bases; a longer one: BMH_EINVAL.  A batch with a query side beyond the aligner's
 * extension cap (bmh_aligner_set_max_qlen; 768 by default) fails the run with BMH_EINVAL naming the cap.  n_threads: host threads of the host forms (<= 0: all).  The aligner borrows idx and pac: both outlive it; popt->rg_id is copied. */
int bmh_effective_cpus(void);      /* CPUs this process may use: affinity mask capped by the cgroup quota (what n_threads <= 0 resolves to) */
typedef struct bmh_aligner bmh_aligner_t;
typedef int (*bmh_sam_sink_t)(void *user, const char *text, size_t len);
typedef struct {
	uint64_t n_reads, n_bytes; uint32_t n_batches; int n_lanes;
	double seconds;                 /* wall clock of the run */
	double format_seconds;          /* in the writer thread (overlaps the workers); a BMH_OUT_BAM_SORTED run adds its final merge, which follows them */
	double h2d_seconds, seed_seconds, chain_extend_seconds, tail_seconds, select_seconds, cigar_seconds;    /* summed over the lanes' host clocks */
	double gate_wait_seconds;       /* lanes waiting for a slot in the path's device stages (ALIGNER_GPU_SLOTS), summed likewise */
	/* the copies themselves, timed by HIP events on the lanes' streams (h2d_seconds / cigar_seconds above are HOST clocks around whole stages: the staging of
	 * letters, offsets and names on host threads; the CIGAR and text kernels the host waits for): reads + offsets + names in, SAM text out */
	double h2d_copy_seconds, d2h_copy_seconds; uint64_t h2d_bytes, d2h_bytes;
} bmh_align_stats_t;
/* Page-locks a caller's host buffer (hipHostRegister) / releases it.  bmh_aligner_run sends the batches of a read set whose letters lie in pinned or registered
 * memory to the device straight from there (no staging copy on host threads). */
int bmh_host_pin(void *p, size_t bytes);
int bmh_host_unpin(void *p);
bmh_aligner_t *bmh_aligner_create(const bmh_index_t *idx, const uint8_t *pac, int64_t l_pac, int n_contigs, const char *const *contig_names,
                                  const int32_t *contig_len, const uint8_t *contig_is_alt, const bmh_chain_opt_t *copt, const bmh_ext_params_t *ep,
                                  const bmh_post_opt_t *popt, const bmh_pe_opt_t *pe);
void bmh_aligner_free(bmh_aligner_t *a);
/* The extension cap of the aligner's chain workspaces (bmh_chain_ws_set_max_qlen): 768 by default, BMH_EXT_LONG_MAX for reads of any length
 * the aligner takes.  Applies to the runs that follow. */
int bmh_aligner_set_max_qlen(bmh_aligner_t *a, uint32_t cap);
/* The seeding rounds of the aligner's lanes (bmh_seed_batch_reseed); NULL = re-seeding off.  Applies to the runs that follow. */
int bmh_aligner_set_reseed(bmh_aligner_t *a, const bmh_reseed_opt_t *opt);
/* Batches of the last run whose region tail the device refused (BMH_ECAPACITY: a patch alignment with a query side beyond 1 022 bases, more than
 * 65 535 near-equal regions; pairs: a read beyond the pairing kernels' limits): the host forms took them, same text. */
uint64_t bmh_aligner_host_tail_batches(const bmh_aligner_t *a);
int bmh_aligner_run(bmh_aligner_t *a, const bmh_read_set_t *reads, const uint64_t *cuts, uint32_t n_batches, int paired, int n_lanes, int n_threads,
                    bmh_sam_sink_t sink, void *user, bmh_align_stats_t *stats);
/* The same from a read FILE (one '>' header line and one sequence line per read, as bmh_reads_load_fasta takes), batch by batch: a loader thread cuts the
 * mapped file the way bseq_read cuts its stream -- reads are added until the batch holds at least batch_bases bases (or exactly batch_reads reads, if that is
 * not 0) and, paired, an even number of reads (src/bwa.c:48-66; the reference's batch_bases is 10 000 000 x its thread count) -- and fills every batch into
 * pinned host memory while the workers are on the batches before it; nothing of the file is held beyond the n_lanes + 3 batches in flight.  Same text as
 * bmh_reads_load_fasta + bmh_aligner_run with the same cuts. */
int bmh_aligner_run_fasta(bmh_aligner_t *a, const char *reads_fa, uint64_t batch_bases, uint64_t batch_reads, int paired, int n_lanes, int n_threads,
                          bmh_sam_sink_t sink, void *user, bmh_align_stats_t *stats);
/* bmh_aligner_run_fasta for a FASTA or FASTQ file (as bmh_reads_load takes it): the loader's pinned batches carry the qualities (QUAL) and, with
 * popt->copy_comment, the comments.  Same text as bmh_reads_load + bmh_aligner_run with the same cuts. */
int bmh_aligner_run_file(bmh_aligner_t *a, const char *path, uint64_t batch_bases, uint64_t batch_reads, int paired, int n_lanes, int n_threads,
                         bmh_sam_sink_t sink, void *user, bmh_align_stats_t *stats);

/* bmh_aligner_run_file for the files bmh_reads_load_files takes (path2: the mates, or NULL; two files imply pairs): a loader thread reads (and inflates) the
 * text into pinned windows, the device cuts them into records, and every batch -- ended as bseq_read ends it -- lands in pinned host memory while the lanes
 * are on the batches before it; at most n_lanes + 3 batches are alive.  Same text as bmh_aligner_run_file on the single-line interleaved file of the same
 * reads.  A file that ends before its mate file: the complete pairs before it are written, then BMH_EINVAL naming the shorter file. */
int bmh_aligner_run_files(bmh_aligner_t *a, const char *path1, const char *path2, uint64_t batch_bases, uint64_t batch_reads, int paired, int n_lanes, int n_threads,
                          bmh_sam_sink_t sink, void *user, bmh_align_stats_t *stats);

/* ---- BAM output: SAM record lines -> BAM records -> BGZF members, on the device (csrc/bam_core.h, csrc/bam_kernels.hip, csrc/deflate_core.h,
 * csrc/deflate_kernels.hip) or by the same two cores as plain C++ on host threads (no device needed).
 *
 * The contig table of both forms: the names NUL-terminated back to back, ctg_name_off [n_contigs + 1] (off[c + 1] - off[c] - 1 = the length of name c).
 * bmh_sam_to_bam_device: the record lines d_text [text_bytes] (every line ends with '\n'; no header lines) on `stream`, which it waits for.  out->d_bam
 * [bam_bytes]: the records back to back in line order; out->d_status [n_records]: 0, or the check that refused the line (bmh_bam_status_name says which:
 * fewer than 11 fields, a name beyond 254 bytes, a bad CIGAR or more than 65 535 operations, a tag that is not XX:T:value with T of A i f Z H, SEQ and QUAL
 * of different lengths, a last line without '\n', an unknown contig, a number outside its range, an integer tag outside [-2^31, 2^32), a float tag that is
 * not [-+]?digits[.digits] of at most 15 digits, a B tag).  A refused line leaves no bytes in d_bam.  The arrays live in the work space until its next call.
 * bmh_sam_to_bam_host: the same from host memory; *bam, *status are malloc'd (bmh_free).
 * bmh_bgzf_deflate_device / _host: the bytes cut into pieces of at most 0xff00, every piece one BGZF member (level 0: a stored block; level 1: LZ77 and
 * dynamic Huffman codes, or the stored block when that is not smaller), back to back; no bytes give no members.  The device and the host form give the
 * same bytes.  bmh_deflate_blocks_host: the members in zeroed slots of 65 536 bytes each, sizes [n_members].  bmh_bgzf_eof: the 28-byte end-of-file member.
 * bmh_bam_header: magic, l_text, the header text, n_ref and the references (malloc'd; bmh_free) -- uncompressed, on the host.
 * bmh_aligner_set_output: what the runs that follow hand to the sink -- BMH_OUT_SAM (the default): the records' text; BMH_OUT_BAM: every batch's records
 * as BGZF members of `level` (0 or 1), the last member of a batch short, so that header members + the batches in order + bmh_bgzf_eof are a BAM file.
 * A record the converter refuses fails the run with a message naming the read. */
typedef struct bmh_bam_ws bmh_bam_ws_t;
typedef struct {
	const uint8_t *d_bam; uint64_t bam_bytes;
	const uint32_t *d_status; uint32_t n_records;
	uint32_t n_refused, first_refused, first_status;       /* how many lines were refused; the first of them and its status */
} bmh_bam_out_t;
#define BMH_OUT_SAM 0
#define BMH_OUT_BAM 1
extern const uint8_t bmh_bgzf_eof[28];
bmh_bam_ws_t *bmh_bam_ws_create(void);
void bmh_bam_ws_free(bmh_bam_ws_t *ws);
int bmh_sam_to_bam_device(bmh_bam_ws_t *ws, const char *d_text, uint64_t text_bytes, int n_contigs, const char *d_ctg_names, const uint32_t *d_ctg_name_off,
                          void *stream, bmh_bam_out_t *out);
int bmh_sam_to_bam_host(const char *text, uint64_t text_bytes, int n_contigs, const char *ctg_names, const uint32_t *ctg_name_off, int n_threads,
                        uint8_t **bam, uint64_t *bam_bytes, uint32_t **status, uint32_t *n_records);
const char *bmh_bam_status_name(uint32_t status);
int bmh_bgzf_deflate_device(bmh_bam_ws_t *ws, const uint8_t *d_in, uint64_t n_bytes, int level, void *stream, const uint8_t **d_out, uint64_t *out_bytes);
int bmh_bgzf_deflate_host(const uint8_t *in, uint64_t n_bytes, int level, int n_threads, uint8_t **out, uint64_t *out_bytes);
int bmh_deflate_blocks_host(const uint8_t *in, uint64_t n_bytes, int level, uint8_t *slots, uint32_t *sizes, int n_threads);
int bmh_bam_header(const char *header_text, int n_contigs, const char *const *contig_names, const int32_t *contig_len, uint8_t **out, uint64_t *out_bytes);
int bmh_aligner_set_output(bmh_aligner_t *a, int format, int level);

/* ---- Coordinate-sorted BAM and its BAI index (csrc/bam_sort_core.h, csrc/bam_sort_kernels.hip, csrc/bam_sort_host.cpp).
 *
 * The order is `samtools sort`'s: key (uint32)refID << 32 | (uint32)(pos + 1) << 1 | reverse strand; records without a reference last; equal keys in the order
 * they came in.  The index is the SAM specification's section 5.2 (bins as the records carry them, the pseudo-bin 37450, the 16 KiB linear index, n_no_coor).
 * bmh_bam_sort_device / _host: a record stream in host memory (whole records, else refused) -> the same records in order (malloc'd; bmh_free).
 * A contig of 2^29 bases or more is refused (BAI cannot index it; a CSI index, below, takes it).
 *
 * One options record and one results record serve every place sorted output is made -- bmh_bam_sorted_file_*, bmh_bam_post_file_* (below) and the aligner's
 * BMH_OUT_BAM_SORTED runs -- and everything it can do there: sort, index, mark duplicates, compute coverage, compute statistics.
 * bmh_sorted_opt_t: the BGZF level (0 or 1); window: records per window of the merge (0: about 64 MiB of records; a window's last member is short); the index
 * (BMH_INDEX_*; min_shift is read for CSI only); sort_mem: record bytes the run store keeps in memory before runs spill to an unnamed file in tmp_dir (0: 4 GiB;
 * NULL: $TMPDIR, else /tmp); markdup, coverage, stats, recal: the options of duplicate marking, coverage, statistics and the recalibration table (the sections
 * below), NULL: off.  recal and the results' recal, recal_ms, recal_windows are the records' last members: code that fills the members before them is unchanged.
 * bmh_sorted_opt_default: level 1, window 0, a BAI index (min_shift 14), the store's defaults, everything off; an opt of NULL means the same.
 * bmh_sorted_results_t: markdup, coverage, stats -- the caller's records, each required exactly when the matching option is set (else BMH_EINVAL) and not read
 * otherwise; the arrays of *coverage and *stats are malloc'd (bmh_free each / bmh_bam_stats_free).  The device milliseconds and the windows timed are filled by
 * aligner runs only: the stand-alone calls time nothing and leave them 0.  results may be NULL where no option asks for a record.
 * Every call zeroes the results and the records they name first, and a failed call leaves *bam, *index (bmh_bam_post_file_*: out's pointers) and every array of
 * *coverage and *stats NULL, whatever they held before: a caller who frees what a failed call left frees nothing.
 * The options are checked in one order, before anything is written: level; the index format and the contigs it can hold; markdup (barcode source, edits, optical
 * step, read groups, then the contigs marking can hold); coverage; stats; recal (its record in the results is required, zeroed and released like theirs).
 * bmh_bam_sorted_file_device / _host: a record stream in host memory -> header members, the sorted records in windows, the end-of-file member; and the .bai or
 * .csi bytes (both malloc'd; bmh_free).  Both forms give the same bytes.  With opt->markdup the stream comes in the writer's order; the optical step is not part
 * of a stand-alone file: optical_distance stays -1, else BMH_EINVAL.  sort_mem and tmp_dir are not read here: the one run stays in memory.
 * bmh_aligner_set_sorted_output: the runs that follow write BMH_OUT_BAM_SORTED under opt (NULL: the defaults).  Every batch becomes a sorted run kept on the host;
 * at the end of the input all runs' keys are sorted once more on the device -- 24 bytes of device memory per record and the sort's work space, fewer than 2^32
 * records, else the run is refused with a message naming the count -- and the sink receives the record members of the sorted file, window after window.  The
 * header members and the end-of-file member stay with the caller.  Everything is checked, in the order above, before anything changes: a refused call leaves the
 * aligner exactly as it was.  Read groups come from bmh_aligner_run_groups or bmh_aligner_set_keep_rg: a markdup record with rg_ids is refused.
 * bmh_aligner_set_output(a, BMH_OUT_BAM_SORTED, level) is bmh_aligner_set_sorted_output with the default record at that level; any other format switches every
 * option of the sorted output off.
 * bmh_aligner_sorted_results: what the last sorted run left.  out->parts: the BMH_SORTED_* parts it computed; n_libraries: the libraries of a marked run over read
 * groups (else 0); the milliseconds -- markdup_ms: the decision (host clock) and the windows' flag steps, markdup_d2h_bytes: the ordinals and entries that came down
 * with the batches, optical_ms: the decision's share that the optical step took, coverage_ms / stats_ms: the windows' steps on the device's stream and the windows
 * timed.  A record of out that is not NULL is filled (lib_counts [8 * n_libraries] and lib_optical [3 * n_libraries], the caller's arrays or NULL; lib_grouped is not
 * written: an aligner run does not count groups per library); it and every part in `need` must be among the parts, else BMH_EINVAL saying which part no run has computed.
 * bmh_aligner_sort_index: the index of the last sorted run (malloc'd; bmh_free); base_offset: the bytes the caller wrote before the sink's first. */
#define BMH_OUT_BAM_SORTED 2
int bmh_bam_sort_device(const uint8_t *records, uint64_t n_bytes, void *stream, uint8_t **out);
int bmh_bam_sort_host(const uint8_t *records, uint64_t n_bytes, uint8_t **out);
typedef struct bmh_markdup_opt bmh_markdup_opt_t;                  /* (below, with duplicate marking, coverage and the statistics) */
typedef struct bmh_markdup_counts bmh_markdup_counts_t;
typedef struct bmh_coverage_opt bmh_coverage_opt_t;
typedef struct bmh_coverage bmh_coverage_t;
typedef struct bmh_bam_stats_opt bmh_bam_stats_opt_t;
typedef struct bmh_bam_stats bmh_bam_stats_t;
typedef struct bmh_recal_opt bmh_recal_opt_t;
typedef struct bmh_recal bmh_recal_t;
typedef struct bmh_recal_apply_opt bmh_recal_apply_opt_t;
typedef struct {
	int32_t level; uint32_t window; int32_t index_format, min_shift;
	uint64_t sort_mem; const char *tmp_dir;
	const bmh_markdup_opt_t *markdup; const bmh_coverage_opt_t *coverage; const bmh_bam_stats_opt_t *stats;
	const bmh_recal_opt_t *recal;
} bmh_sorted_opt_t;
#define BMH_SORTED_MARKDUP 1u
#define BMH_SORTED_OPTICAL 2u
#define BMH_SORTED_BARCODE 4u
#define BMH_SORTED_GROUPED 8u
#define BMH_SORTED_COVERAGE 16u
#define BMH_SORTED_STATS 32u
#define BMH_SORTED_RECAL 64u
typedef struct {
	bmh_markdup_counts_t *markdup; bmh_coverage_t *coverage; bmh_bam_stats_t *stats;
	uint32_t parts; int32_t n_libraries;
	double markdup_ms[2], optical_ms, coverage_ms, stats_ms; uint64_t markdup_d2h_bytes, coverage_windows, stats_windows;
	bmh_recal_t *recal; double recal_ms; uint64_t recal_windows;
} bmh_sorted_results_t;
void bmh_sorted_opt_default(bmh_sorted_opt_t *o);
int bmh_bam_sorted_file_device(const char *header_text, int n_contigs, const char *const *contig_names, const int32_t *contig_len, const uint8_t *records, uint64_t n_bytes,
                               const bmh_sorted_opt_t *opt, void *stream, uint8_t **bam, uint64_t *bam_bytes, uint8_t **index, uint64_t *index_bytes, bmh_sorted_results_t *results);
int bmh_bam_sorted_file_host(const char *header_text, int n_contigs, const char *const *contig_names, const int32_t *contig_len, const uint8_t *records, uint64_t n_bytes,
                             const bmh_sorted_opt_t *opt, uint8_t **bam, uint64_t *bam_bytes, uint8_t **index, uint64_t *index_bytes, bmh_sorted_results_t *results);
int bmh_aligner_set_sorted_output(bmh_aligner_t *a, const bmh_sorted_opt_t *opt);
int bmh_aligner_sorted_results(bmh_aligner_t *a, bmh_sorted_results_t *out, uint32_t need);
int bmh_aligner_sort_index(bmh_aligner_t *a, uint64_t base_offset, uint8_t **bai, uint64_t *bai_bytes);

/* ---- A CSI index in place of the BAI, for contigs of 2^29 bases and more (BAM holds positions up to 2^31 - 1; only BAI's bins stop at 2^29).  Opt-in: without
 * it every byte is as before.  The binning scheme is (min_shift, depth): min_shift from the caller (10 .. 24, else refused; 14 is BAI's), depth the smallest d with
 * 2^(min_shift + 3 d) >= the longest contig, as htslib chooses it.  A record's bin is that of the deepest level that holds its first and last 2^min_shift window
 * (pos < 0 counts as 0, a record running off its contig is clamped to the contig's last window); the record's own 16-bit bin field is neither read nor changed, so the
 * BAM bytes are those of the BAI call.  The .csi bytes, little-endian, as BGZF members and the end-of-file member:
 *   "CSI\1"  int32 min_shift  int32 depth  int32 l_aux = 0  int32 n_ref
 *   per reference: int32 n_bin, then per bin, ascending, the pseudo-bin ((1 << 3 (depth + 1)) - 1) / 7 + 1 last:
 *     uint32 bin  uint64 loffset  int32 n_chunk  n_chunk x (uint64 beg, uint64 end)
 *   uint64 n_no_coor
 * loffset: the smallest begin offset over the records that overlap the bin's first window, or, if none does, the next window that has one; 0 for the pseudo-bin,
 * whose two chunks are (first begin, last end) and (mapped, unmapped).  A reference without records has n_bin 0.
 * index_format BMH_INDEX_CSI and min_shift in bmh_sorted_opt_t ask for it; the contig lengths are checked against the format where the options are (BAI: below
 * 2^29; CSI: at most 2^31 - 1, and an index of fewer than 2^28 windows).  bmh_aligner_sort_index gives the bytes of the format the last sorted run was made under.
 * For BMH_INDEX_BAI min_shift is not read.
 * Duplicate marking holds an unclipped end in 31 bits around 2^30: with it on, a contig beyond 2^30 - 2^24 bases is refused by name before anything is written. */
#define BMH_INDEX_BAI 0
#define BMH_INDEX_CSI 1

/* ---- Duplicate marking in sorted BAM (csrc/bam_dup_core.h, csrc/bam_dup_kernels.hip, csrc/bam_dup_host.cpp).
 * Picard MarkDuplicates' rules on templates (a single read or a read pair, its records next to each other in the writer's order): the unclipped 5' ends and
 * strands of the primary lines are the key, the sum of the base qualities >= 15 the score, ties go to the template that came first in the input; a fragment is
 * a duplicate wherever a pair has an end.  Every record of a duplicate template gets flag 0x400.  Nothing is removed; optical duplicates are counted on request (below).  One library unless
 * read groups are given (below).
 * counts [8]: pairs examined, fragments examined, duplicate pairs, duplicate fragments, records flagged, secondary or supplementary records, unmapped records,
 * templates.
 * One options record and one counts record serve every stand-alone marking call; the sections below say what each field means.  bmh_markdup_opt_default: no read
 * groups, no optical step (-1, 0), no barcodes (0, -1, 0).  The counts record is zeroed by every call; lib_counts [8 * n_lib], lib_optical [3 * n_lib] and
 * lib_grouped [3 * n_lib] are the caller's arrays (or NULL), filled with read groups only.
 * bmh_bam_markdup_device / _host: a record stream in the writer's order (whole records; the first begins a template; paired templates hold both primary lines --
 * else BMH_EINVAL with a message) -> the same records with the flags set (malloc'd; bmh_free).  opt NULL: plain marking; res is required.
 * bmh_sorted_opt_t's markdup: the duplicates of a sorted output marked under the same record, its counts in the results' markdup. */
struct bmh_markdup_opt {
	const char *const *rg_ids; const int32_t *rg_lib; int32_t n_groups;   /* all NULL / 0: no read groups */
	int64_t  optical_distance;      /* -1: no optical step */
	uint64_t optical_max_set;       /* 0: the default (300 000) */
	int32_t  barcode_mode;          /* 0 off, 1 tag, 2 read name */
	char     barcode_tag[2];
	int32_t  barcode_edits;         /* -1: barcodes compared exactly */
	uint64_t barcode_max_set;       /* 0: the default (65 536) */
};
void bmh_markdup_opt_default(bmh_markdup_opt_t *o);
struct bmh_markdup_counts {
	uint64_t counts[8], optical[3], grouped[3], no_barcode;
	uint64_t *lib_counts, *lib_optical, *lib_grouped;   /* caller's arrays [8 | 3 | 3 per library], or NULL */
};
int bmh_bam_markdup_device(const uint8_t *records, uint64_t n_bytes, const bmh_markdup_opt_t *opt, void *stream, uint8_t **out, bmh_markdup_counts_t *res);
int bmh_bam_markdup_host(const uint8_t *records, uint64_t n_bytes, const bmh_markdup_opt_t *opt, uint8_t **out, bmh_markdup_counts_t *res);
int bmh_aligner_set_bam_pairs(bmh_aligner_t *a, uint64_t batch_bases, int n_lanes);        /* (described with bmh_bam_reads_device above) */
int bmh_aligner_set_collate(bmh_aligner_t *a, int on, uint64_t mem_bytes);                  /* (described with bmh_reads_last_collate_counts above) */
/* Keep the input's read groups (off by default; with it off nothing about a run changes).  bmh_aligner_run_files then takes one BAM -- a regular file or a pipe --
 * whose header's @RG lines are the run's read groups, in file order (bmh_bam_header_read_groups' rules and refusals), and every read's records carry RG:Z:<the ID its
 * own record names> where popt->rg_id's tag goes: the decoder gives every read its group (bmh_bam_reads_groups_device's rules and refusals), a batch holds reads of
 * any number of groups and is cut as without the option, and a read's index (the tie-break hash) is its index in the file.  `header` is called once, after the
 * input's header has been read whole and before the first call of the sink: rg_lines holds the @RG lines verbatim, each with a '\n' behind it -- what the caller
 * writes into its output header --, lib [n_groups] every group's library (bmh_bam_header_read_groups); a non-zero return ends the run.  A refused header ends the
 * run before either is called.  With BMH_OUT_BAM_SORTED and duplicate marking the duplicates are called within a library and bmh_aligner_sorted_results gives
 * a row per library.  Refused: text input, a mates file, an aligner with a read group of its own (popt->rg_id), bmh_aligner_run_groups (keep-rg and a run over
 * groups do not combine), more than 255 libraries with duplicate marking. */
typedef int (*bmh_rg_header_fn)(void *user, const char *rg_lines, size_t len, int n_groups, const int32_t *lib);
int bmh_aligner_set_keep_rg(bmh_aligner_t *a, int on, bmh_rg_header_fn header, void *user);

/* ---- Read groups and libraries.
 * Duplicates per library: rg_ids [n_groups] and rg_lib [n_groups] are the run's read groups and every group's library index (0 .. 254; groups with one index are
 * lanes of one library).  A template's library is that of the RG:Z tag on its first record; pairs are duplicates of each other, a fragment is a duplicate through a
 * pair's end, and the best fragment stays, within one library only.  The library takes the top byte of the duplicate key, above the refID: more than 255 libraries,
 * a refID of 2^24 or more, an empty table, an empty ID and two rows with one ID are refused (BMH_EINVAL) before anything is allocated; so is a template whose first
 * record has no RG:Z tag or names a group the table does not hold, by the record's index.  counts [8]: the totals, as without groups.  lib_counts (or NULL)
 * [8 * n_lib], n_lib = 1 + the largest index: the same eight per library.  Without groups no tag is read. */

/* ---- Optical duplicates and the library-size estimate (csrc/bam_dup_core.h).  Counts only: the records, the flags, the file and its index are
 * byte for byte those of the call without the option (Picard flags nothing more for an optical duplicate by default).
 * A template's location is (tile, x, y): the last three of the 5 or 7 ':'-separated fields of its first record's read name, each the field's leading run of digits
 * (a value below 2^31; what follows the digits is ignored); any other name has none.  Among the pairs of one duplicate key -- a set, the pair that stays included --
 * two located pairs are neighbours when read group, role (which mate holds the smaller end), and tile are equal and x and y each differ by at most `distance`;
 * the connected components are the clusters and a cluster of k pairs counts k - 1 optical duplicates.  Sets of one pair and sets of more than max_set pairs
 * (0: 300 000) are not examined.  optical [3]: optical duplicate pairs, examined pairs with a location, sets skipped for their size; lib_optical (or NULL)
 * [3 * n_lib]: the same per library.  distance: 0 .. 2^31 - 1.
 * With an optical distance a run holds at most 65536 read groups.
 * bmh_bam_dup_locations_device / _host: a record stream -> *locs: one 16-byte location per template {int32 x, y; uint32 tile; uint16 group row; uint16 flags --
 * 1: located, 2: role} (malloc'd; bmh_free), *n_templates of them.
 * bmh_bam_name_location: the parser on the host -> 1 and out = {tile, x, y}, or 0: no location.
 * bmh_library_size: Picard's estimateLibrarySize of n_pairs pairs that are no optical duplicates, n_unique of them distinct -> 1 and *size, or 0: no estimate. */
int bmh_bam_dup_locations_device(const uint8_t *records, uint64_t n_bytes, const char *const *rg_ids, const int32_t *rg_lib, int n_groups, void *stream, uint8_t **locs,
                                 uint64_t *n_templates);
int bmh_bam_dup_locations_host(const uint8_t *records, uint64_t n_bytes, const char *const *rg_ids, const int32_t *rg_lib, int n_groups, uint8_t **locs, uint64_t *n_templates);
int bmh_bam_name_location(const char *name, uint32_t len, uint32_t out[3]);
int bmh_library_size(uint64_t n_pairs, uint64_t n_unique, int64_t *size);

/* ---- Barcode-aware duplicate keys (UMIs; csrc/bam_dup_core.h).  Opt-in: without it every output byte is that of the calls above.
 * A template's barcode comes from its first record -- the record its library and its location come from.  barcode_mode 1 (a tag): the value of tag `tag` (two
 * characters, [A-Za-z][A-Za-z0-9]; not RG, nor one the aligner writes itself: NM MD AS XS SA XA pa) of type Z, verbatim -- no case folding, no splitting at '-'.
 * barcode_mode 2 (the name): the bytes behind the last ':' of the read name (bcl-convert's ...:tile:x:y:UMI); the optical step's parser is then given the name
 * without that field and its ':'.  0: none (tag ignored).  An absent tag, an empty value, a name without ':' and a name that ends in ':' mean no barcode: such
 * templates are comparable with each other and with no barcoded one; no_barcode counts them.  The value becomes a 64-bit word -- FNV-1a over its
 * bytes, 0 kept for no barcode (a value that hashes to 0 takes 1) -- and words are compared: pairs by (lo, hi, word), fragments by (end, word), a fragment a
 * duplicate through a pair's end only if that pair has its word, an optical set the pairs of one (lo, hi, word).  Refused with BMH_EINVAL and the record's index: a
 * first record whose tag has a type other than Z, or whose tags cannot be walked.
 * bmh_bam_dup_barcodes_device / _host: a record stream -> *words: one uint64 per template (malloc'd; bmh_free), *n_templates of them; barcode_mode 1 or 2; packed
 * != 0: the packed words that grouping by edits compares (below).
 * bmh_barcode_word: the word of a value of n bytes.
 * A tag reaches the records of an aligner run only as a read's comment (-C). */
int bmh_bam_dup_barcodes_device(const uint8_t *records, uint64_t n_bytes, int barcode_mode, const char tag[2], int packed, void *stream, uint64_t **words, uint64_t *n_templates);
int bmh_bam_dup_barcodes_host(const uint8_t *records, uint64_t n_bytes, int barcode_mode, const char tag[2], int packed, uint64_t **words, uint64_t *n_templates);
uint64_t bmh_barcode_word(const uint8_t *value, uint64_t n);

/* ---- Barcodes grouped within an edit distance (csrc/bam_dup_core.h).  Opt-in beside a barcode source: `edits` N (0 .. 21; -1: off, the calls
 * above) makes barcodes within N mismatches one molecule, as Picard's UmiAwareMarkDuplicatesWithMateCigar (MAX_EDIT_DISTANCE_TO_JOIN) does.  The barcode word is then
 * the value itself, packed: 3 bits a byte -- A 1, C 2, G 3, T 4, N 5, '-' 6, '+' 7 --, symbol i in bits 3 i .. 3 i + 2, at most 21 symbols, 0 still no barcode.
 * The distance of two words is the number of positions at which their symbols differ; values of different lengths are never joined, nor is a template without a
 * barcode to one with.  Within one (library, lo, hi) the distinct words of the pairs are clustered -- connected components of distance <= N, so joining is
 * transitive -- and every pair takes its component's smallest word; the pair rule then runs on (lo, hi, that word), and an optical set is the pairs of one such
 * key.  Independently, within one (library, end word) the distinct words of the fragment pass's items -- the fragments and both ends of every pair -- are
 * clustered the same way before the fragment rule.  A key with more than barcode_max_set distinct words (0: 65 536) is not clustered: its words stay exact.  With
 * N = 0 flags and counts are those of the exact comparison.  grouped [3], lib_grouped [3 * libraries] (or NULL; filled with read groups): the distinct
 * (library, lo, hi, word) over barcoded pairs, their components, and the keys of either pass over the cap.
 * Refused with BMH_EINVAL before anything is written: edits outside -1 .. 21, edits without a barcode source; and by the record's index: a first record whose
 * value holds more than 21 bytes or a byte other than A C G T N - + (lower case too).
 * bmh_barcode_pack: *word of a value of n bytes; 1, or 0 when it does not pack. */
int bmh_barcode_pack(const uint8_t *value, uint64_t n, uint64_t *word);

/* A run over several read groups: one sample's lanes and libraries into one output.  A group is a read group ID, its library index (as above) and an input as
 * bmh_aligner_run_files takes it (path2: the mates, or NULL; a BAM's own @RG lines and RG tags stay ignored: keeping the input's read groups, bmh_aligner_set_keep_rg, and a run over groups do not combine).  One loader thread walks the groups in order into the
 * one queue of batches: the lanes are not drained between groups.  A batch never spans two groups and is cut inside its group as bmh_aligner_run_files cuts it; the
 * read index behind the tie-break hash restarts at 0 in every group; every record carries its group's ID as RG:Z.  So group g's records are byte for byte those of
 * bmh_aligner_run_files on its input alone by an aligner whose read group is g's, and the unsorted output is the groups' outputs in order.  Sorted output with
 * duplicate marking decides per library; the template ordinal behind its tie-break counts on across the groups (the input order of the whole run).
 * All groups hold pairs or none does (two files, `paired`, or a BAM whose first kept record has flag 0x1 mean pairs): a group that disagrees is refused by its ID
 * when the loader reaches it -- the groups before it have been written by then, as with a file that ends before its mate file.  When no group has two files, paired
 * is 0 and the first group is a BAM that holds pairs, the run takes bmh_aligner_set_bam_pairs' values as bmh_aligner_run_files does.  Refused before anything is
 * written: n_groups < 1, an aligner created with a read group of its own (popt->rg_id), an empty ID or one beyond 255 bytes, two groups with one ID, a library
 * index outside 0 .. 254, a path that does not exist.  Messages about a file or a read name the group's ID, and the read by its index within its group. */
typedef struct { const char *id; int32_t library; const char *path1, *path2; } bmh_read_group_t;
int bmh_aligner_run_groups(bmh_aligner_t *a, const bmh_read_group_t *groups, int n_groups, uint64_t batch_bases, uint64_t batch_reads, int paired, int n_lanes,
                           int n_threads, bmh_sam_sink_t sink, void *user, bmh_align_stats_t *stats);

/* ---- Coverage depth of sorted BAM, computed while the file is written (csrc/bam_cov_core.h, csrc/bam_cov_kernels.hip, csrc/bam_cov_host.cpp).
 * A record counts when its refID names a contig, none of the flags 0x4 0x100 0x200 0x400 is set and mapq >= min_mapq (`samtools depth`'s default filters;
 * supplementary records count).  It covers the reference positions under M, = and X, and under D with `deletions` (`samtools depth -J`); N never covers.  A run past
 * the contig's end is clamped; a counted record without operations is a read that covers nothing.  No base-quality filter, no correction for overlapping mates.
 * The results are exact integers and do not depend on windows, tiles or the form: per contig n_reads (counted records), cov_bases (positions of depth >= 1),
 * sum_depth, max_depth and sum_mapq (over counted records); hist [1001]: the positions of all contigs at depth d, hist[1000] those at 1000 and more, depth 0
 * included, so the bins add up to the genome; with bin = B >= 1, bin_sum [n_bins]: the depth summed over every B positions of a contig (its last bin short),
 * contig after contig.  tile: the positions swept through one difference array (1 .. 4096; 0: 4096); work and memory follow the covered runs, not the genome.
 * All arrays of bmh_coverage_t are malloc'd: bmh_free each (a failed call leaves them NULL).
 * bmh_bam_coverage_device / _host: a record stream in coordinate order (whole records, else refused).  Both forms give the same integers.
 * Refused with BMH_EINVAL: min_mapq outside 0 .. 255, a tile beyond 4096, 2^28 bins or more (before anything is written); and by the record's index: a record
 * that lies before its predecessor, a counted record whose pos is negative or not below its contig's length, a counted record that holds the long-CIGAR
 * placeholder (l_seq S, N, and a CG:B,I tag).
 * bmh_sorted_opt_t's coverage: the coverage of a sorted output from the windows of its merge, every window behind its flag step -- duplicates that markdup marks
 * are counted out.  Without it nothing about a run changes.  An aligner run times its windows' steps and its last sweep on the device's stream (events around
 * every step, read behind the window's own wait; a step's span holds its two host reads): coverage_ms, coverage_windows. */
struct bmh_coverage_opt { int32_t min_mapq, deletions; uint32_t bin; uint32_t tile; };
void bmh_coverage_opt_default(bmh_coverage_opt_t *o);
struct bmh_coverage {
	int32_t n_contigs; uint64_t n_bins;
	uint64_t *n_reads, *cov_bases, *sum_depth, *max_depth, *sum_mapq;   /* [n_contigs] each */
	uint64_t *hist;                                                      /* [1001] */
	uint64_t *bin_sum;                                                   /* [n_bins] */
};
int bmh_bam_coverage_device(const uint8_t *records, uint64_t n_bytes, int n_contigs, const int32_t *contig_len, const bmh_coverage_opt_t *opt, void *stream, bmh_coverage_t *out);
int bmh_bam_coverage_host(const uint8_t *records, uint64_t n_bytes, int n_contigs, const int32_t *contig_len, const bmh_coverage_opt_t *opt, bmh_coverage_t *out);

/* ---- Sort, mark duplicates and index a BAM or SAM that any aligner wrote (csrc/bam_post_core.h, csrc/bam_post_kernels.hip, csrc/bam_post.cpp).
 * No index and no aligner handle: the input (a regular file or a pipe; BAM -- BGZF whose text begins "BAM\1" -- or SAM text, plain, gzip or BGZF, told apart by
 * their bytes) is read in order, inflated on host threads, cut into batches of about batch_bytes record bytes that end where a read name ends, and every batch
 * becomes a sorted run as a batch of the aligner does; at the end of the input the runs are merged into the coordinate-sorted file (header members, record
 * members in windows, the end-of-file member: all of it goes to the sink) with its index, the duplicates marked, the coverage and the statistics
 * computed as a BMH_OUT_BAM_SORTED run does it -- the same calls underneath, so this aligner's own unsorted BAM or SAM gives byte for byte the file of its
 * sorted run.
 * The header's text is the input's with every @HD line removed and "@HD\tVN:1.6\tSO:coordinate\n" in front, nothing else added; the references are the BAM's
 * binary table, or the SAM's @SQ lines (SN, LN) in order -- a SAM without one is refused.  Records stay verbatim but for the bin (recomputed: reg2bin(pos, end),
 * 4680 for pos -1) and, with marking, flag 0x400 (cleared first, then set by the decision).  Equal keys stay in input order over the whole file.
 * A template is a maximal run of adjacent records under one read name, in any order inside it (BDP_TPL_NAME); its ordinal is its place in the input.
 * Refused with BMH_EINVAL, by the record's index in the file (SAM: the line's number), the smallest first, before anything is written: a record that is not
 * whole; refID or next_refID outside -1 .. n_ref - 1; a SAM line the converter refuses (bmh_bam_status_name's words); with marking: the primary lines of a paired
 * name that are not one 0x40 and one 0x80 record (a file that is not grouped by name, such as a coordinate-sorted one), a mapped primary line with refID or pos
 * -1, an unclipped 5' end u with u + 2^30 outside [0, 2^31); with marking or coverage: a record that holds the long-CIGAR placeholder.  The contig-length
 * refusals of the sorted output hold (BAI below 2^29, marking at most 2^30 - 2^24, the CSI window count).  The result does not depend on batch_bytes, window,
 * sort_mem or spilling.
 * opt (NULL: the defaults): sorted -- the record of every sorted output (above), read whole; batch_bytes (0: 256 MiB; at most 1 GiB); libraries != 0 (needs
 * sorted.markdup, whose rg_ids stay NULL): the header's @RG lines are the table of libraries, by bmh_bam_header_read_groups' rules with markdup on, and the
 * results' markdup->lib_* (or NULL) then hold room for 255 libraries.
 * out (zeroed first; bmh_bam_post_result_free releases it; a refused call leaves its pointers NULL): the index bytes, the output header's text, the references
 * (names NUL-terminated back to back), with libraries their names likewise, and the counts: records, templates, batches, runs spilled, records whose bin
 * changed, records whose 0x400 was cleared.  results: as above.
 * The host form does the same with the host forms of every step and no device; it holds the whole record stream in memory.
 * collate != 0 (needs markdup, else BMH_EINVAL before anything is read; off by default, and with it off every byte, count and message is as without the field):
 * templates by name over the whole file (BDP_TPL_FILE), so that a coordinate-sorted file can be marked.  A template is the records of the whole file that carry
 * one read name, adjacent or not; its first record is the one with the smallest file index (library, barcode and location come from it), its ordinal the rank of
 * that record among all first records; its entry is bdp_entry's rule on the set (n_rec the set's size, the two mapped primary lines in file order).  A set that
 * is no proper template -- a paired one whose primary lines are not one 0x40 and one 0x80 record, an unpaired one without exactly one primary line, so also two
 * templates under one name anywhere in the file -- is refused with BMH_EINVAL naming its first record's index (and the SAM line) and the primary lines found;
 * of all refusals of first records and of sets the smallest (index, code) is reported, after the last batch and before the header reaches the sink.  Names are
 * keyed by 128 bits (FNV-1a and a second hash) and never compared byte by byte; a collision merges two whole templates into an improper set, which is refused.
 * Batches then end at the first record at or beyond batch_bytes.  Every record's 32-byte part (48 or 56 with optical_distance / barcodes) stays in host memory
 * until the grouping: about 32 GB for 10^9 records, outside sort_mem, never spilled.  On a name-grouped file with distinct names the output is byte for byte
 * that of collate 0. */
typedef struct { bmh_sorted_opt_t sorted; uint64_t batch_bytes; int32_t libraries, collate; } bmh_bam_post_opt_t;
typedef struct { uint64_t records, templates, batches, spilled_runs, bins_changed, dup_flags_cleared; } bmh_bam_post_counts_t;
typedef struct {
	uint8_t *index; uint64_t index_bytes;
	char *header_text; uint64_t header_bytes;
	int32_t n_contigs; char *contig_names; int32_t *contig_len;
	int32_t n_libraries; char *library_names;
	bmh_bam_post_counts_t counts;
} bmh_bam_post_result_t;
void bmh_bam_post_opt_default(bmh_bam_post_opt_t *o);
void bmh_bam_post_result_free(bmh_bam_post_result_t *r);
int bmh_bam_post_file_device(const char *path, const bmh_bam_post_opt_t *opt, void *stream, bmh_sam_sink_t sink, void *user, bmh_bam_post_result_t *out,
                             bmh_sorted_results_t *results);
int bmh_bam_post_file_host(const char *path, const bmh_bam_post_opt_t *opt, bmh_sam_sink_t sink, void *user, bmh_bam_post_result_t *out, bmh_sorted_results_t *results);
/* The grouping of collate on its own (csrc/bam_tpl_core.h, csrc/bam_tpl_kernels.hip, csrc/bam_tpl_host.cpp): a stream of whole BAM records in any order -> every
 * record's template ordinal (tpl [n_records]), the templates' entries (24 bytes each: uint64 lo, hi; uint32 score, kind | records << 2), their locations (16
 * bytes each: int32 x, y; uint32 tile; uint16 rg, flags), with opt's barcode source their barcode words, counts: secondary or supplementary records, unmapped
 * records, templates; with opt's read groups the three per library (lib_counts [3 * n_libraries]).  opt (NULL: plain): the read groups, the barcode source and
 * barcode_edits (packed words) are read.  hash_bits: 128; below it the name keys are cut, so that a test can make two names collide.  Records go through the
 * per-record checks of marking first; an improper set and a refused first record give BMH_EINVAL as under collate.  bmh_bam_templates_free releases *out. */
typedef struct {
	uint64_t n_records, n_templates;
	uint32_t *tpl; uint8_t *entries, *locs; uint64_t *barcodes;
	uint64_t counts[3]; uint64_t *lib_counts; int32_t n_libraries;
} bmh_bam_templates_t;
int bmh_bam_templates_device(const uint8_t *records, uint64_t n_bytes, const bmh_markdup_opt_t *opt, int32_t hash_bits, void *stream, bmh_bam_templates_t *out);
int bmh_bam_templates_host(const uint8_t *records, uint64_t n_bytes, const bmh_markdup_opt_t *opt, int32_t hash_bits, bmh_bam_templates_t *out);
void bmh_bam_templates_free(bmh_bam_templates_t *r);

/* ---- Flag counts, contig counts, an alignment summary and insert sizes of sorted BAM, computed while the file is written (csrc/bam_stats_core.h,
 * csrc/bam_stats_kernels.hip, csrc/bam_stats_host.cpp): what `samtools flagstat`, `samtools idxstats` and an insert-size summary would read the
 * file again for.  Every word is an exact uint64 over the whole file and does not depend on the order of the records, on windows or on the form.
 * flag [2][16]: `samtools flagstat`'s counts, column 0 the records without 0x200 and column 1 those with it, in the order total, primary, secondary,
 * supplementary, duplicates, primary duplicates, mapped, primary mapped, paired, read1, read2, properly paired, with itself and mate mapped, singletons, mate on a
 * different contig, that at mapq >= 5.  A record with 0x100 and 0x800 is secondary only; proper and singleton need 0x4 clear.
 * contig_mapped / contig_unmapped [n_contigs], unplaced: `samtools idxstats`' counts over records of every kind -- refID c without and with 0x4, refID -1.
 * summary [14], over primary records (neither 0x100 nor 0x800): reads, bases (l_seq), reads mapped, bases mapped (0x4 clear), mapped reads at mapq 0, the longest
 * l_seq; and of the mapped ones, from the operations: bases aligned (M = X I), bases soft-clipped, insertion events and bases, deletion events and bases; from the
 * tags: records with NM, and the sum of NM (the first NM of a record, of type c C s S i I).  mapq [256]: the mapped primary records by mapq.
 * insert_hist [3][insert_cap + 1] (FR, RF, TANDEM), insert_min / insert_max [3]: Picard CollectInsertSizeMetrics' rule at its defaults, once per pair -- a record
 * with 0x1 and 0x80, none of 0x4 0x8 0x100 0x800 0x400, refID == next_refID and tlen != 0 counts with the size |tlen|; TANDEM when 0x10 and 0x20 are equal, else a
 * forward record is FR with tlen > 0 and a reverse record is FR with next_pos + 1 < pos + its reference length, RF otherwise.  Sizes from insert_cap (2 .. 65536;
 * the default 65536) up share the last bin; the smallest and the largest size are exact (0 where an orientation holds no pair).
 * Refused with BMH_EINVAL by the record's index: a refID outside -1 .. n_contigs - 1; of mapped primary records (no other record's operations or tags are read)
 * tags that cannot be walked to the record's end, an NM of another type or below 0, the long-CIGAR placeholder.  The first such record is the one named.
 * bmh_bam_stats_device / _host: a record stream in any order (whole records, else refused).  bmh_bam_stats_free releases the arrays (a failed call leaves them NULL).
 * bmh_sorted_opt_t's stats: the statistics of a sorted output from the windows of its merge, every window behind its flag step, with the 0x400 flags markdup
 * sets.  Without it no run launches anything more.  An aligner run times its windows' kernels on the device's stream: stats_ms, stats_windows. */
struct bmh_bam_stats_opt { uint32_t insert_cap; };
void bmh_bam_stats_opt_default(bmh_bam_stats_opt_t *o);
struct bmh_bam_stats {
	int32_t n_contigs; uint32_t insert_cap;
	uint64_t *flag;                                                      /* [2][16] */
	uint64_t *summary;                                                   /* [14] */
	uint64_t *mapq;                                                      /* [256] */
	uint64_t *contig_mapped, *contig_unmapped;                           /* [n_contigs] each */
	uint64_t *insert_hist;                                               /* [3][insert_cap + 1] */
	uint64_t unplaced, insert_min[3], insert_max[3];
};
void bmh_bam_stats_free(bmh_bam_stats_t *s);
int bmh_bam_stats_device(const uint8_t *records, uint64_t n_bytes, int n_contigs, const bmh_bam_stats_opt_t *opt, void *stream, bmh_bam_stats_t *out);
int bmh_bam_stats_host(const uint8_t *records, uint64_t n_bytes, int n_contigs, const bmh_bam_stats_opt_t *opt, bmh_bam_stats_t *out);

/* ---- The covariate table of base quality score recalibration, counted while sorted BAM is written (csrc/bam_recal_core.h, csrc/bam_recal_kernels.hip,
 * csrc/bam_recal_host.cpp): what GATK BaseRecalibrator's counting pass would read the file again for, at its default covariates (read group,
 * quality, cycle, context) with BAQ off.  DESIGN.md 4.16 holds the definition and the differences from GATK (no adaptor-boundary clipping, no low-quality-tail
 * masking of contexts, no BAQ, cycles above the cap binned, the output is this project's text); nothing here has been compared with GATK itself.
 * bmh_recal_opt_t: min_qual (0 .. 93; default 6), max_cycle (1 .. 65535; default 500); the reference -- pac: the .pac body on the host (forward strand, 4 bases a
 * byte), l_pac its bases, contig_offset [n_contigs] every contig's first base in it (NULL: the contigs back to back); an aligner run reads the index's own copy on
 * the device when pac is NULL.  mask [mask_words] (or NULL): bit i & 63 of word i >> 6 masks base i (bmh_known_sites_mask, bmh_recal_mask_holes); mask_words is
 * (l_pac + 63) / 64.  rg_ids [n_groups]: the read groups in table order (at most 255); 0 groups: every record belongs to the one group `*` and RG tags are not read.
 * bmh_recal_t: summary [16] -- records seen, counted, left out (no contig, flags, mapq, no qualities, no operations), bases kept, bases skipped (no ACGT, quality
 * below min_qual, masked position, masked insertion anchor), cycles capped, masked positions; cycle_m [groups][94][2 max_cycle][2] (observations, errors of event M;
 * slot max_cycle + c - 1 for cycle c > 0, max_cycle + c for c < 0), cycle_id [groups][2 max_cycle][3] (observations of I and of D -- one word --, insertion errors,
 * deletion errors, at quality 45), context_m [groups][94][17][2] (context 4 a + b; 16: none), context_id [groups][65][3] (16 a + 4 b + c; 64: none).
 * The accumulator holds at most 2^28 words (groups x max_cycle is bounded by that), else BMH_EINVAL.
 * Refused with BMH_EINVAL by the record's index, the smallest first: see DESIGN.md 4.16.  bmh_recal_free releases the arrays (a failed call leaves them NULL).
 * bmh_bam_recal_device / _host: a record stream in any order.  bmh_sorted_opt_t's recal: the table of a sorted output from the windows of its merge, every
 * window behind its flag step.  Without it no run launches anything more.
 * bmh_known_sites_mask: text files, plain or gzip, VCF (first non-empty line begins ##fileformat=VCF or #CHROM: a data line masks [POS - 1, POS - 1 + len(REF)))
 * or BED ([start, end); track, browser and # lines ignored) -> bits OR-ed into mask; refused naming file and line: an unknown contig, a position outside its
 * contig, too few fields, a number that does not parse.  bmh_recal_mask_holes: the reference's holes (.amb: offset, length pairs in pac) OR-ed into the mask. */
struct bmh_recal_opt {
	int32_t min_qual, max_cycle;
	const uint8_t *pac; uint64_t l_pac; const uint64_t *contig_offset;
	const uint64_t *mask; uint64_t mask_words;
	int32_t n_groups; const char *const *rg_ids;
	const bmh_recal_apply_opt_t *apply;   /* the table to apply to the qualities as they are written (below); NULL: off */
	int32_t no_count;                     /* read with apply only.  1: apply only -- no table is counted, pac, mask, the contigs' places and rg_ids are not read */
};
void bmh_recal_opt_default(bmh_recal_opt_t *o);
struct bmh_recal {
	int32_t n_groups, min_qual, max_cycle, n_qual;
	uint64_t summary[16];
	uint64_t *cycle_m, *cycle_id, *context_m, *context_id;
	/* the apply step's members: read and written only where the options' apply is set (bmh_bam_requal_*: always) */
	uint64_t apply_summary[16];
	uint64_t *qual_hist;
	double apply_ms; uint64_t apply_windows;
};
void bmh_recal_free(bmh_recal_t *r);
void bmh_recal_kernel_limits(uint32_t out[5]);   /* the device form's capacities: slots, lanes per record, cycles per LDS row, records per block, bases per LDS record */
int bmh_bam_recal_device(const uint8_t *records, uint64_t n_bytes, int n_contigs, const int32_t *contig_len, const bmh_recal_opt_t *opt, void *stream, bmh_recal_t *out);
int bmh_bam_recal_host(const uint8_t *records, uint64_t n_bytes, int n_contigs, const int32_t *contig_len, const bmh_recal_opt_t *opt, bmh_recal_t *out);
int bmh_known_sites_mask(const char *const *paths, int n_paths, int n_contigs, const char *const *contig_names, const int32_t *contig_len, const uint64_t *contig_offset,
                         uint64_t *mask, uint64_t mask_words);
int bmh_recal_mask_holes(const uint64_t *hole_offset, const uint64_t *hole_len, int n_holes, uint64_t *mask, uint64_t mask_words);

/* ---- Applying a recalibration table to the base qualities while sorted BAM is written (csrc/bam_requal_core.h, csrc/bam_requal.h, csrc/bam_requal_kernels.hip;
 * DESIGN.md 4.17): the step that follows the table -- this project's restatement of GATK ApplyBQSR's hierarchical delta model over event M (group, quality, cycle,
 * context), with the plain empirical quality -10 log10((errors + 1) / (observations + 2)).  It was not compared with GATK.  Not done: an OQ tag, quantised
 * output qualities, insertion and deletion qualities, GATKReport files, counting and applying one table in one run, the Bayesian empirical quality.
 * bmh_recal_apply_opt_t: table -- a bmh_recal_t of counts as the counting pass returns it (n_groups, min_qual, max_cycle, n_qual, cycle_m and context_m are read);
 * rg_ids [table->n_groups] its read groups' IDs (NULL, or the one ID `*`: the table's one group applies to every record and RG tags are not read).
 * Refused before anything is written, naming the row: errors above observations, a (group, quality) whose cycle rows and context rows sum differently (the slot
 * `none` included), min_qual or max_cycle out of range.  Refused by the record's index, the smallest of a window first: a record that is not whole; with groups
 * tags that cannot be walked, no RG tag, an RG tag of another type than Z, an ID the table does not hold.
 * Every record with qualities is rewritten, whatever its flags; a quality below the table's min_qual stays; nothing else in a record changes.
 * bmh_recal_opt_t's apply: the step in every window of a sorted output behind the flag step and in front of coverage, statistics, the counting of a table
 * (which then counts the qualities as written) and the compressor; the results' bmh_recal_t holds apply_summary -- records seen, rewritten, without qualities;
 * bases seen, below min_qual, changed, unchanged; cycles capped, bases without context --, qual_hist [2][94] (the qualities before and after; malloc'd, released by
 * bmh_recal_free), the kernels' milliseconds and the windows timed.  Both members are the options' last, the apply members the record's last: a caller who built
 * either before they existed, positionally or zeroed, leaves apply NULL, and then no byte of the record beyond cycle .. context_id is read or written.
 * (summary [15] of a record that holds the apply members is 1: that is how bmh_recal_free knows.)
 * bmh_recal_apply_tables: the int16 deltas both forms read -- [groups][94][1 + 2 max_cycle + 16]: b, the cycle deltas, the context deltas, in 1/256 of a quality
 * (malloc'd; bmh_free).  bmh_bam_requal_device / _host: a record stream -> the same stream with the qualities rewritten (malloc'd; bmh_free) and the counts; both
 * forms give the same bytes.  bmh_requal_kernel_limits: lanes per record, records per block, bases of a record whose counts stay in LDS. */
struct bmh_recal_apply_opt {
	const bmh_recal_t *table;
	const char *const *rg_ids;
};
int bmh_recal_apply_tables(const bmh_recal_apply_opt_t *apply, int16_t **tables, uint64_t *n_entries);
int bmh_bam_requal_device(const uint8_t *records, uint64_t n_bytes, const bmh_recal_apply_opt_t *apply, void *stream, uint8_t **out, bmh_recal_t *counts);
int bmh_bam_requal_host(const uint8_t *records, uint64_t n_bytes, const bmh_recal_apply_opt_t *apply, uint8_t **out, bmh_recal_t *counts);
void bmh_requal_kernel_limits(uint32_t out[3]);

#ifdef __cplusplus
}
#endif
#endif
