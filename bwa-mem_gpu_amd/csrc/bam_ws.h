// The device work space of the BAM output path (csrc/bam_kernels.hip, csrc/deflate_kernels.hip): buffers that only grow, kept between batches.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string>
#include "bmh_internal.h"
#include "devmem.h"

struct bmh_bam_ws {
	// records: newlines per chunk and their scan, line ends, sizes, statuses, offsets, the records, the scans' scratch, counters
	dev_buf<uint8_t> cnt, cnt_off, line_end, size, status, off, bam, tmp, flags;
	// members: slots, sizes, offsets, the members back to back
	dev_buf<uint8_t> slots, msize, moff, members, mtmp;
};

// csrc/bam_kernels.hip: the name of record `rec` of the text the work space has just converted (for messages)
std::string bmh_bam_record_name_device(bmh_bam_ws_t *ws, const char *d_text, uint64_t text_bytes, uint32_t rec);
