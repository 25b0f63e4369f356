// bmh_format_sam_parts (csrc/sam_format.cpp: the host formatter as the native pipeline calls it) over 32-bit slots and the packed words of bmh_cigar_pack,
// behind a C function for tests/test_sam_core.py.  Host code only, linked against libbwamem_hip.so.
#include <cstdlib>
#include <cstring>
#include "../bwa-mem_gpu_amd/csrc/bmh_internal.h"

extern "C" char *sam_parts_packed(const bmh_post_opt_t *po, uint32_t n_reads, const char *names, const uint64_t *name_off, const uint8_t *reads, const uint64_t *read_offs,
                                  const uint32_t *read_lens, const uint8_t *quals, const char *comments, const uint64_t *comment_off, int n_contigs,
                                  const char *const *contig_names, const int64_t *contig_offset, const int32_t *fin, const uint32_t *fin_per_read, const int32_t *h_rec,
                                  const int32_t *unflag, const int32_t *slot32, const int32_t *aln, const uint32_t *off, const uint32_t *packed, size_t *len_out)
{
	std::vector<std::string> parts;
	bmh_cigar_src_t cs;
	cs.slot32 = slot32; cs.aln = aln; cs.packed = packed; cs.off = off;
	if (!bmh_format_sam_parts(po, n_reads, names, name_off, reads, read_offs, read_lens, n_contigs, contig_names, contig_offset, fin, fin_per_read, cs, h_rec, unflag, parts,
	                          quals, comments, comment_off)) return nullptr;
	std::string all;
	for (const std::string &p : parts) all += p;
	char *res = (char *)malloc(all.size() + 1);
	memcpy(res, all.c_str(), all.size() + 1);
	*len_out = all.size();
	return res;
}
