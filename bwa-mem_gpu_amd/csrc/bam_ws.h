// The device work space of the BAM output path (csrc/bam_kernels.hip, csrc/deflate_kernels.hip): buffers that only grow, kept between batches.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string>
#include "bmh_internal.h"

struct bmh_grow_t {
	void *p = nullptr; size_t cap = 0;
	bmh_grow_t() = default;
	bmh_grow_t(const bmh_grow_t &) = delete;
	bmh_grow_t &operator=(const bmh_grow_t &) = delete;
	int need(size_t bytes)
	{
		if (bytes <= cap) return BMH_OK;
		if (p) (void)hipFree(p);
		p = nullptr; cap = 0;
		const size_t c = bytes + bytes / 4 + 1024;
		if (hipMalloc(&p, c) != hipSuccess) { bmh_set_error("BAM output: %zu bytes of device memory: %s", c, hipGetErrorString(hipGetLastError())); p = nullptr; return BMH_ENOMEM; }
		cap = c;
		return BMH_OK;
	}
	~bmh_grow_t() { if (p) (void)hipFree(p); }
};

struct bmh_bam_ws {
	// records: newlines per chunk and their scan, line ends, sizes, statuses, offsets, the records, the scans' scratch, counters
	bmh_grow_t cnt, cnt_off, line_end, size, status, off, bam, tmp, flags;
	// members: slots, sizes, offsets, the members back to back
	bmh_grow_t slots, msize, moff, members, mtmp;
};

// csrc/bam_kernels.hip: the name of record `rec` of the text the work space has just converted (for messages)
std::string bmh_bam_record_name_device(bmh_bam_ws_t *ws, const char *d_text, uint64_t text_bytes, uint32_t rec);
