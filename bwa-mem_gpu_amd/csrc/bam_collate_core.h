// Mates collated by name over a stream of BAM records (--collate): the definition both forms of the BAM decoder follow (csrc/reads_io.cpp: bmh_bam_host_run walks
// it record by record; csrc/bam_in_kernels.hip matches a window's names by hash, sort and scan and must give the same), compiled as plain C++ by
// tests/bam_collate_host.cpp (under the sanitizers).
//
//   Kept records (no flag 0x100 / 0x800) are taken in file order.  A record whose name is open closes that record: the two are a pair, completed at the later
//   record's index; two records of one role under one open name are refused.  Any other record opens its name.  The reads are the pairs in the order of their
//   completion; at the file's end an open record is refused (the one with the smallest index is named).  Skipped records open and close nothing.
//
// A window is consumed up to the record that completes the last pair taken from it.  The open records inside that prefix move into the pool below, which outlives
// the window: their bytes in host memory, each with its index in the file; the records behind the prefix stay in the window and are walked again.  Nothing is
// changed before a window delivers (bcl_walk_t::deliver): a window that holds no complete batch is read on and walked anew.
//   open records / open bytes   the table of the definition: the pool's records and the window's open ones; a record counts 4 + block_size bytes
//   cap                         the open bytes are held against it at every completion: the pair is refused, naming the first record since the completion before
//                               it that took the open bytes beyond the cap (so the records behind the file's last completion are never counted: they are refused
//                               as records without partner).  Batches that were complete before that record have been delivered.
#pragma once
#include <stdint.h>
#include <string.h>
#include <algorithm>
#include <string>
#include <unordered_map>
#include <unordered_set>
#include <vector>
#include "bam_in_core.h"
#include "bam_dup_core.h"

// what bmh_reads_last_collate_counts reports (include/bwamem_hip.h: bmh_collate_counts_t has the same five words)
struct bcl_counts_t { uint64_t pairs = 0, pairs_adjacent = 0, open_records_peak = 0, open_bytes_peak = 0, windows_to_host_for_hash_runs = 0; };

// the key of a name of n bytes (without its NUL): 64-bit FNV-1a, cut to its low `bits` bits (COLLATE_HASH_BITS below 64 forces equal keys for the tests)
BSR_FN uint64_t bcl_hash(const uint8_t *name, uint32_t n, int bits)
{
	const uint64_t h = bdp_fnv1a64(name, n);
	return bits >= 64 ? h : h & ((1ull << bits) - 1);
}

// ---- the pool of open records
struct bcl_slot_t { std::vector<uint8_t> bytes; uint64_t index = 0, hash = 0; bool used = false; };
struct bcl_pool_t {
	std::vector<bcl_slot_t> slots; std::vector<uint32_t> free_slots;      // a freed slot is the next one taken
	std::unordered_map<std::string, uint32_t> by_name;
	uint64_t cap = 8ull << 30, bytes = 0, n = 0, version = 0;            // version: every change counts (the device form's resident keys follow it)
	int hash_bits = 64;
	bool ended_open = false;                                            // the run was refused for a record still open at the file's end (the complete pairs stay delivered)
	bcl_counts_t cnt;

	const char *name(uint32_t s) const { return (const char *)slots[s].bytes.data() + BI_NAME_OFF; }
	uint32_t role(uint32_t s) const { return bi_role(bi_u16(slots[s].bytes.data() + 18)); }
	int64_t find(const std::string &nm) const { auto it = by_name.find(nm); return it == by_name.end() ? -1 : (int64_t)it->second; }
	uint32_t add(const uint8_t *rec, uint32_t size, uint64_t index)
	{
		uint32_t s;
		if (!free_slots.empty()) { s = free_slots.back(); free_slots.pop_back(); }
		else { s = (uint32_t)slots.size(); slots.emplace_back(); }
		bcl_slot_t &e = slots[s];
		e.bytes.assign(rec, rec + size); e.index = index; e.used = true;
		const uint32_t ln = rec[12];
		e.hash = bcl_hash(rec + BI_NAME_OFF, ln - 1, hash_bits);
		by_name[std::string((const char *)rec + BI_NAME_OFF)] = s;
		bytes += size; ++n; ++version;
		return s;
	}
	void remove(uint32_t s)
	{
		bcl_slot_t &e = slots[s];
		by_name.erase(std::string(name(s)));
		bytes -= e.bytes.size(); --n; ++version;
		std::vector<uint8_t>().swap(e.bytes); e.used = false;
		free_slots.push_back(s);
	}
	int64_t smallest() const                                            // the open record with the smallest index (walked at a refusal only)
	{
		int64_t b = -1;
		for (size_t s = 0; s < slots.size(); ++s) if (slots[s].used && (b < 0 || slots[s].index < slots[(size_t)b].index)) b = (int64_t)s;
		return b;
	}
};

// ---- one window walked by the definition
enum { BCL_OPENED = 0, BCL_PAIR = 1, BCL_SAME_ROLE = 2, BCL_OVER_CAP = 3 };
// the record a name was open as: in the pool (slot) or in the window (rec); bytes / size: the record itself; index: its index in the file
struct bcl_partner_t { bool in_pool; uint32_t slot, rec, size, role; uint64_t index; const uint8_t *bytes; };

struct bcl_walk_t {
	bcl_pool_t &P; const uint8_t *buf; const uint32_t *starts; uint64_t base;      // base: the file index of the window's record 0
	struct wrec_t { uint32_t rec, size, role; uint64_t seq; };
	std::unordered_map<std::string, wrec_t> wopen;                       // the window's open records
	std::unordered_set<uint32_t> closed;                                 // pool slots closed by this window
	uint64_t cur_n, cur_b, pk_n, pk_b, seq = 0, pairs = 0, adjacent = 0;
	int64_t over_at = -1;                                                // the first record since the last completion that took the open bytes beyond the cap
	bool committed = false; uint32_t c_rec = 0; uint64_t c_pk_n = 0, c_pk_b = 0;

	bcl_walk_t(bcl_pool_t &pool, const uint8_t *b, const uint32_t *st, uint64_t first) : P(pool), buf(b), starts(st), base(first), cur_n(pool.n), cur_b(pool.bytes), pk_n(pool.n), pk_b(pool.bytes) {}

	// the kept record `rec` of the window (role 1 or 2).  BCL_OPENED; BCL_PAIR and *pt: its partner, closed -- the caller emits the pair and calls commit(rec);
	// BCL_SAME_ROLE and *pt: the open record of the same role; BCL_OVER_CAP and pt->index: the record that went beyond the cap
	int step(uint32_t rec, uint32_t role, bcl_partner_t *pt)
	{
		const uint8_t *r = buf + starts[rec];
		const uint32_t size = starts[rec + 1] - starts[rec];
		const std::string nm((const char *)r + BI_NAME_OFF);
		const uint64_t my_seq = seq++;
		auto wo = wopen.find(nm);
		int64_t s = -1;
		if (wo == wopen.end()) { s = P.find(nm); if (s >= 0 && closed.count((uint32_t)s)) s = -1; }
		if (wo == wopen.end() && s < 0) {
			wopen[nm] = wrec_t{rec, size, role, my_seq};
			++cur_n; cur_b += size;
			pk_n = std::max(pk_n, cur_n); pk_b = std::max(pk_b, cur_b);
			if (cur_b > P.cap && over_at < 0) over_at = (int64_t)(base + rec);
			return BCL_OPENED;
		}
		if (wo != wopen.end()) { const wrec_t &o = wo->second; *pt = bcl_partner_t{false, 0, o.rec, o.size, o.role, base + o.rec, buf + starts[o.rec]}; }
		else { const bcl_slot_t &e = P.slots[(size_t)s]; *pt = bcl_partner_t{true, (uint32_t)s, 0, (uint32_t)e.bytes.size(), P.role((uint32_t)s), e.index, e.bytes.data()}; }
		if (over_at >= 0) { pt->index = (uint64_t)over_at; return BCL_OVER_CAP; }
		if (pt->role == role) return BCL_SAME_ROLE;
		if (wo != wopen.end()) { if (wo->second.seq + 1 == my_seq) ++adjacent; wopen.erase(wo); }
		else closed.insert((uint32_t)s);
		--cur_n; cur_b -= pt->size; ++pairs;
		return BCL_PAIR;
	}
	// the pair completed at `rec` has been emitted: the window can be consumed up to here
	void commit(uint32_t rec) { committed = true; c_rec = rec; c_pk_n = pk_n; c_pk_b = pk_b; }
	// the window delivers its pairs and is consumed behind record c_rec: closed slots leave the pool, the open records up to c_rec enter it (in file order)
	void deliver()
	{
		if (!committed) return;
		for (uint32_t s : closed) P.remove(s);
		std::vector<uint32_t> in;
		for (const auto &kv : wopen) if (kv.second.rec <= c_rec) in.push_back(kv.second.rec);
		std::sort(in.begin(), in.end());
		for (uint32_t rec : in) P.add(buf + starts[rec], starts[rec + 1] - starts[rec], base + rec);
		P.cnt.pairs += pairs; P.cnt.pairs_adjacent += adjacent;
		P.cnt.open_records_peak = std::max(P.cnt.open_records_peak, c_pk_n); P.cnt.open_bytes_peak = std::max(P.cnt.open_bytes_peak, c_pk_b);
	}
	// the window's own open record with the smallest index, or -1
	int64_t first_open() const { int64_t b = -1; for (const auto &kv : wopen) if (b < 0 || kv.second.rec < (uint32_t)b) b = kv.second.rec; return b; }
	bool open_behind_commit() const { for (const auto &kv : wopen) if (!committed || kv.second.rec > c_rec) return true; return false; }
};
