// Coverage depth, internal: the plan and the host form (csrc/bam_cov_host.cpp) and what csrc/bam_cov_kernels.hip offers csrc/bam_sort_kernels.hip and
// csrc/align_pipeline.hip.  Both forms take the sorted file's windows of records one after the other and keep the same state between them: the events at or
// behind the frontier (the tile that holds the last record's start: later records may still add to it), the depth carried into the first position not yet
// added, and that position.
#pragma once
#include <stdint.h>
#include <vector>
#ifndef BCV_STANDALONE
#include "bmh_internal.h"
#else                                                              // tests/bam_cov_core_host.cpp: the host form alone, without the library
enum { BMH_OK = 0, BMH_EINVAL = -2, BMH_ENOMEM = -4 };
void bmh_set_error(const char *fmt, ...);
#endif
#include "bam_cov_core.h"

// what a coverage run is made under, checked: the options (tile: the positions of a tile, the default filled in), the contigs' lengths and offsets, the bins' places
struct bcv_plan_t {
	int32_t min_mapq = 0; bool deletions = false; uint64_t bin = 0, tile = BCV_TILE_DEFAULT;
	int n_contigs = 0;
	std::vector<int64_t> len; std::vector<uint64_t> coff, bin_off;      // [n], [n + 1], [n + 1]
	uint64_t genome() const { return coff.back(); }
	uint64_t n_bins() const { return bin_off.back(); }
};
// min_mapq, deletions, bin, tile as the entry points take them (tile 0: the default).  Refused (BMH_EINVAL, a message): min_mapq outside 0 .. 255, a tile beyond
// BCV_TILE_MAX, a negative contig length, 2^28 bins or more
int bcv_plan_make(bcv_plan_t &P, int32_t min_mapq, int32_t deletions, uint32_t bin, uint32_t tile, int n_contigs, const int32_t *contig_len, const char *fn);

// the results: five words per contig, the histogram, the bins
struct bcv_result_t {
	std::vector<uint64_t> n_reads, cov_bases, sum_depth, max_depth, sum_mapq, hist, bin_sum;
	void init(const bcv_plan_t &P);
	// depth 0 in closed form: the genome's positions that no other bin holds
	void close(const bcv_plan_t &P);
};

// the message of the record with index `rec` that bcv_check refuses (st), or that lies before its predecessor (st -1)
int bcv_refused(uint64_t rec, int st, const char *fn);

// the host form
struct bcv_host_t {
	bcv_plan_t P; bcv_result_t R;
	std::vector<uint64_t> pending;                                     // event keys at or behind the frontier's tile
	uint64_t carry = 0, done_to = 0, n_seen = 0, last_key = 0;        // depth at done_to, the first position not added yet; records so far, the last one's sort key
	std::vector<int64_t> diff;
	void begin(const bcv_plan_t &plan);
	// a window's n records recs + soff[j] in coordinate order (checked: a record before its predecessor is refused by its index)
	int window(const uint8_t *recs, const uint64_t *soff, uint32_t n, const char *fn);
	// the end of the stream: everything is added, R is complete
	int finish(const char *fn);
private:
	void sweep(uint64_t frontier);
	void add(uint64_t a, uint64_t b, uint64_t d, int &c);             // positions [a, b) of one contig at depth d > 0; c: the contig of the position before (a cursor)
};

#ifndef BCV_STANDALONE
struct bmh_coverage;
// R as the entry points return it (malloc'd arrays; *out zeroed first)
int bcv_export(const bcv_plan_t &P, const bcv_result_t &R, struct bmh_coverage *out, const char *fn);

// csrc/bam_cov_kernels.hip
struct bcv_dev_t;                                                  // the device form's buffers and state; one per sorted run
bcv_dev_t *bcv_dev_create(void);
void bcv_dev_free(bcv_dev_t *d);
int bcv_begin_device(bcv_dev_t *d, const bcv_plan_t &P, void *stream);
// a window's records d_recs at d_soff [n + 1] (device) in coordinate order; last: the window's last record (host), which sets the frontier.  With ms (or NULL)
// events are recorded around the step; bcv_window_ms reads them once the caller has waited for the stream: ms[0] += the milliseconds from the step's first kernel to
// its last (its two host reads lie in between), ms[1] += 1 (the windows timed)
int bcv_window_device(bcv_dev_t *d, const uint8_t *d_recs, const uint64_t *d_soff, uint32_t n, const uint8_t *last, void *stream, const char *fn, double *ms);
int bcv_window_ms(bcv_dev_t *d, double *ms);
// the last sweep (ms[0] += its milliseconds) and the results
int bcv_finish_device(bcv_dev_t *d, void *stream, bcv_result_t &R, const char *fn, double *ms);
#endif
