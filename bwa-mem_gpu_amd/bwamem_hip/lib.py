"""ctypes binding of libbwamem_hip.so (include/bwamem_hip.h, include/seed_gen.h)."""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

_PKG = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_u8p, _u32p, _u64p, _i32p = (C.POINTER(t) for t in (C.c_uint8, C.c_uint32, C.c_uint64, C.c_int32))


class HipLibraryMissing(RuntimeError):
    pass


def lib_path() -> str:
    # BMH_LIB: another build of the same library (A/B runs of kernel variants, scripts/build_variants.sh)
    return os.environ.get("BMH_LIB") or os.path.join(_PKG, "libbwamem_hip.so")


# every symbol include/bwamem_hip.h and include/seed_gen.h declare
EXPORTED_SYMBOLS = [
    "bmh_last_error", "bmh_device_count", "bmh_set_device", "bmh_index_upload", "bmh_index_from_device",
    "bmh_index_free", "bmh_index_kbits_info", "bmh_index_probe", "bmh_index_replicate", "bmh_rccl_where", "bmh_rccl_unique_id", "bmh_rccl_comm_init_rank", "bmh_rccl_comm_destroy", "bmh_index_broadcast_rccl", "bmh_index_replicate_all", "bmh_shard_range", "bmh_index_densify_sa", "bmh_index_build", "bmh_seed_ws_create", "bmh_seed_ws_free", "bmh_seed_batch", "bmh_seed_last_timing", "bmh_seed_ws_set_sample", "bmh_seeds_sample_state", "bmh_seeds_locate_all", "bmh_reseed_opt_default", "bmh_seed_batch_reseed", "bmh_reseed_last_counts", "bmh_aligner_set_reseed",
    "bmh_host_pin", "bmh_host_unpin", "bmh_extend_batch", "bmh_extend_batch_long", "bmh_extend_last_ms", "bmh_extend_last_unsupported", "bmh_extend_last_class_sizes", "bmh_extend_set_packed", "bmh_tune_set", "bmh_wtrace_start", "bmh_wtrace_stop", "bmh_wtrace_kept", "bmh_extend_release", "bmh_finalize_release", "bmh_matesw_release", "bmh_calib_gather", "bmh_calib_valu", "bmh_calib_valu_placed", "bmh_calib_last_clock",
    "bmh_jobs_frac_rep", "bmh_post_opt_default", "bmh_finalize_regs", "bmh_finalize_regs_device", "bmh_finalize_regs_device_last_ms", "bmh_finalize_regs_device_last_classes", "bmh_sam_need_cigar", "bmh_format_sam", "bmh_free",
    "bmh_pe_opt_default", "bmh_finalize_pairs", "bmh_finalize_pairs_dev", "bmh_dedup_regs_device", "bmh_finalize_pairs_deduped", "bmh_rescue_check_counts", "bmh_sam_need_cigar_pe", "bmh_format_sam_pe",
    "bmh_chain_opt_default", "bmh_chain_last_timing", "bmh_build_jobs", "bmh_jobs_free", "bmh_jobs_sizes", "bmh_jobs_arrays", "bmh_merge_regs",
    "bmh_chain_ws_create", "bmh_chain_ws_free", "bmh_chain_set_contigs", "bmh_chain_set_alt", "bmh_effective_cpus", "bmh_aligner_create", "bmh_aligner_free", "bmh_aligner_run", "bmh_aligner_run_fasta", "bmh_chain_set_materialize", "bmh_chain_batch",
    "bmh_chain_extend", "bmh_chain_merge", "bmh_chain_extend_merge", "bmh_chain_extend_merge_timing", "bmh_chain_class_counts", "bmh_cigar_batch", "bmh_cigar_release",
    "bmh_sam_select_work", "bmh_sam_select_device", "bmh_cigar_pack_work", "bmh_cigar_pack_sizes", "bmh_cigar_pack", "bmh_sam_text_work", "bmh_sam_text_sizes", "bmh_sam_text_write", "bmh_sam_text_check",
    "bwt_destroy_gpu", "bwt_restore_sa_gpu", "bwt_restore_bwt_gpu", "gpu_cpy_wrapper",
    "pre_calc_seed_intervals_wrapper", "free_gpuseed_data", "seed_gpu", "seed_gpu_last_n_reads",
    "bmh_reads_load_fasta", "bmh_reads_free", "bmh_fasta_scan",
    "bmh_reads_load", "bmh_reads_scan", "bmh_format_sam_ex", "bmh_format_sam_pe_ex", "bmh_aligner_run_file",
    "bmh_chain_ws_set_max_qlen", "bmh_aligner_set_max_qlen", "bmh_aligner_host_tail_batches",
    "bmh_index_fasta", "bmh_fasta_pack", "bmh_fasta_packed_free",
    "bmh_reads_load_files", "bmh_aligner_run_files",
    "bmh_bgzf_scan", "bmh_inflate_members_device", "bmh_inflate_members_host", "bmh_inflate_status_name", "bmh_bgzf_inflate",
    "bmh_bam_ws_create", "bmh_bam_ws_free", "bmh_sam_to_bam_device", "bmh_sam_to_bam_host", "bmh_bam_status_name", "bmh_bgzf_deflate_device", "bmh_bgzf_deflate_host",
    "bmh_deflate_blocks_host", "bmh_bam_header", "bmh_aligner_set_output",
    "bmh_bam_sort_device", "bmh_bam_sort_host", "bmh_sorted_opt_default", "bmh_bam_sorted_file_device", "bmh_bam_sorted_file_host", "bmh_aligner_set_sorted_output", "bmh_aligner_sorted_results", "bmh_aligner_sort_index",
    "bmh_bam_reads_device", "bmh_bam_reads_host", "bmh_reads_last_bam_counts", "bmh_aligner_set_bam_pairs",
    "bmh_markdup_opt_default", "bmh_bam_markdup_device", "bmh_bam_markdup_host", "bmh_aligner_run_groups",
    "bmh_bam_reads_groups_device", "bmh_bam_reads_groups_host", "bmh_bam_header_read_groups", "bmh_format_sam_groups", "bmh_aligner_set_keep_rg",
    "bmh_bam_dup_locations_device", "bmh_bam_dup_locations_host", "bmh_bam_name_location", "bmh_library_size",
    "bmh_bam_dup_barcodes_device", "bmh_bam_dup_barcodes_host", "bmh_barcode_word", "bmh_barcode_pack",
    "bmh_reads_last_collate_counts", "bmh_aligner_set_collate", "bmh_reads_load_files_ex", "bmh_bam_reads_ex",
    "bmh_coverage_opt_default", "bmh_bam_coverage_device", "bmh_bam_coverage_host",
    "bmh_bam_stats_opt_default", "bmh_bam_stats_free", "bmh_bam_stats_device", "bmh_bam_stats_host",
    "bmh_bam_post_opt_default", "bmh_bam_post_result_free", "bmh_bam_post_file_device", "bmh_bam_post_file_host",
    "bmh_bam_templates_device", "bmh_bam_templates_host", "bmh_bam_templates_free",
    "bmh_recal_opt_default", "bmh_recal_free", "bmh_recal_kernel_limits", "bmh_bam_recal_device", "bmh_bam_recal_host", "bmh_known_sites_mask", "bmh_recal_mask_holes",
    "bmh_recal_apply_tables", "bmh_bam_requal_device", "bmh_bam_requal_host", "bmh_requal_kernel_limits",
]


class SamDev(C.Structure):
    """bmh_sam_dev_t: device pointers of bmh_sam_text_sizes / bmh_sam_text_write"""
    _fields_ = [("n_reads", C.c_uint32), ("d_names", C.c_void_p), ("d_name_off", C.c_void_p), ("d_reads", C.c_void_p), ("d_offs", C.c_void_p), ("d_lens", C.c_void_p),
                ("n_contigs", C.c_int), ("d_contig_names", C.c_void_p), ("d_contig_name_off", C.c_void_p), ("d_contig_offset", C.c_void_p),
                ("d_fin", C.c_void_p), ("d_fin_per_read", C.c_void_p), ("d_slot", C.c_void_p), ("d_aln", C.c_void_p), ("d_cig_off", C.c_void_p), ("d_packed", C.c_void_p),
                ("d_h_rec", C.c_void_p), ("d_unflag", C.c_void_p), ("d_quals", C.c_void_p), ("d_comments", C.c_void_p), ("d_comment_off", C.c_void_p),
                ("d_read_group", C.c_void_p), ("d_rg_ids", C.c_void_p), ("d_rg_id_off", C.c_void_p), ("n_rg", C.c_uint32)]


class ReadGroupsT(C.Structure):
    """bmh_read_groups_t: a read group per read for bmh_format_sam_groups"""
    _fields_ = [("read_group", C.c_void_p), ("ids", C.c_void_p), ("id_off", C.c_void_p), ("n_groups", C.c_uint32)]


def _rg_id_table(ids):
    """read group IDs -> (the IDs back to back as a uint8 array, their offsets [n + 1] as uint32): the table bmh_read_groups_t and bmh_sam_dev_t take"""
    enc = [(i if isinstance(i, bytes) else str(i).encode()) for i in ids]
    return np.frombuffer(b"".join(enc) or b"\0", dtype=np.uint8).copy(), np.concatenate([[0], np.cumsum([len(e) for e in enc])]).astype(np.uint32)


class ReadSetT(C.Structure):
    """bmh_read_set_t"""
    _fields_ = [("n_reads", C.c_uint64), ("n_bases", C.c_uint64), ("n_name_bytes", C.c_uint64), ("ascii", C.c_void_p), ("codes", C.c_void_p),
                ("offs", C.c_void_p), ("lens", C.c_void_p), ("names", C.c_void_p), ("name_offs", C.c_void_p),
                ("quals", C.c_void_p), ("comments", C.c_void_p), ("comment_offs", C.c_void_p), ("n_comment_bytes", C.c_uint64), ("groups", C.c_void_p)]


class _ReadSetOwner:
    """keeps a bmh_read_set_t alive for the numpy arrays that look into it; frees it with the last of them"""

    def __init__(self, L, rs):
        self.L, self.rs = L, rs

    def __del__(self):
        try:
            self.L.bmh_reads_free(C.byref(self.rs))
        except Exception:
            pass


def fasta_scan(path: str, n_threads: int = 0) -> dict:
    """bmh_fasta_scan: reads / bases / name bytes / longest read of a read file, from one counting pass (nothing is loaded)"""
    L = load_library()
    L.bmh_fasta_scan.restype = C.c_int
    L.bmh_fasta_scan.argtypes = [C.c_char_p, C.c_int, C.POINTER(C.c_uint64)]
    out = (C.c_uint64 * 4)()
    rc = L.bmh_fasta_scan(path.encode(), n_threads, out)
    if rc != 0:
        raise RuntimeError(f"bmh_fasta_scan rc={rc}: " + _err(L))
    return dict(n_reads=int(out[0]), n_bases=int(out[1]), n_name_bytes=int(out[2]), max_len=int(out[3]))


def load_fasta_reads(path: str, n_threads: int = 0) -> dict:
    """bmh_reads_load_fasta: the read file as numpy arrays over the library's own arrays (no copies; freed with the last array)"""
    L = load_library()
    rs = ReadSetT()
    L.bmh_reads_load_fasta.argtypes = [C.c_char_p, C.c_int, C.POINTER(ReadSetT)]
    L.bmh_reads_free.argtypes = [C.POINTER(ReadSetT)]
    if L.bmh_reads_load_fasta(path.encode(), n_threads, C.byref(rs)) != 0:
        msg = _err(L)
        raise ValueError(msg) if "expected alternating" in msg else RuntimeError("bmh_reads_load_fasta: " + msg)
    owner = _ReadSetOwner(L, rs)

    def arr(ptr, n, dt):
        n = int(n)
        if n == 0 or not ptr:
            return np.zeros(0, dt)
        buf = (C.c_uint8 * (n * np.dtype(dt).itemsize)).from_address(ptr)
        buf._owner = owner
        return np.frombuffer(buf, dtype=dt)
    return dict(ascii=arr(rs.ascii, rs.n_bases, np.uint8), codes=arr(rs.codes, rs.n_bases, np.uint8), offs=arr(rs.offs, rs.n_reads, np.uint64),
                lens=arr(rs.lens, rs.n_reads, np.uint32), names=arr(rs.names, rs.n_name_bytes, np.uint8), name_offs=arr(rs.name_offs, rs.n_reads, np.uint64))


READS_COMMENTS = 1          # BMH_READS_COMMENTS


class ReadFileError(ValueError, RuntimeError):
    """a malformed read file (bmh_reads_load, bmh_reads_scan, bmh_aligner_run_file): a ValueError whose message names the problem, and a
    RuntimeError as the FASTA-only entry points' refusals were"""


def reads_scan(path: str, n_threads: int = 0) -> dict:
    """bmh_reads_scan: fasta_scan for a FASTA or FASTQ file"""
    L = load_library()
    L.bmh_reads_scan.restype = C.c_int
    L.bmh_reads_scan.argtypes = [C.c_char_p, C.c_int, C.POINTER(C.c_uint64)]
    out = (C.c_uint64 * 4)()
    if L.bmh_reads_scan(path.encode(), n_threads, out) != 0:
        msg = _err(L)
        raise ReadFileError(msg) if msg.startswith(("FASTQ:", "reads file:")) else RuntimeError("bmh_reads_scan: " + msg)
    return dict(n_reads=int(out[0]), n_bases=int(out[1]), n_name_bytes=int(out[2]), max_len=int(out[3]))


def load_reads(path: str, comments: bool = False, n_threads: int = 0) -> dict:
    """bmh_reads_load: a FASTA or FASTQ file as load_fasta_reads gives it, plus quals (FASTQ; None for FASTA) and, with comments=True, the header
    comments (comments / comment_offs: NUL-terminated back to back like the names).  A malformed file raises ValueError naming the problem."""
    L = load_library()
    rs = ReadSetT()
    L.bmh_reads_load.argtypes = [C.c_char_p, C.c_int, C.c_int, C.POINTER(ReadSetT)]
    L.bmh_reads_free.argtypes = [C.POINTER(ReadSetT)]
    if L.bmh_reads_load(path.encode(), n_threads, READS_COMMENTS if comments else 0, C.byref(rs)) != 0:
        msg = _err(L)
        raise ReadFileError(msg) if msg.startswith(("FASTQ:", "reads file:")) else RuntimeError("bmh_reads_load: " + msg)
    owner = _ReadSetOwner(L, rs)

    def arr(ptr, n, dt):
        n = int(n)
        if n == 0 or not ptr:
            return np.zeros(0, dt)
        buf = (C.c_uint8 * (n * np.dtype(dt).itemsize)).from_address(ptr)
        buf._owner = owner
        return np.frombuffer(buf, dtype=dt)
    return dict(ascii=arr(rs.ascii, rs.n_bases, np.uint8), codes=arr(rs.codes, rs.n_bases, np.uint8), offs=arr(rs.offs, rs.n_reads, np.uint64),
                lens=arr(rs.lens, rs.n_reads, np.uint32), names=arr(rs.names, rs.n_name_bytes, np.uint8), name_offs=arr(rs.name_offs, rs.n_reads, np.uint64),
                quals=arr(rs.quals, rs.n_bases, np.uint8) if rs.quals else None,
                comments=arr(rs.comments, rs.n_comment_bytes, np.uint8) if rs.comments else None,
                comment_offs=arr(rs.comment_offs, rs.n_reads, np.uint64) if rs.comments else None)


READS_HOST = 2              # BMH_READS_HOST
READS_COLLATE = 4           # BMH_READS_COLLATE


class CollateCountsT(C.Structure):
    """bmh_collate_counts_t"""
    _fields_ = [(n, C.c_uint64) for n in ("pairs", "pairs_adjacent", "open_records_peak", "open_bytes_peak", "windows_to_host_for_hash_runs")]


def reads_last_collate_counts() -> dict:
    """bmh_reads_last_collate_counts: what the collation of mates by name (collate=True) did in the process's last load_reads_files / bam_reads / run_files /
    run_groups call -- pairs, the pairs whose two records were adjacent, the peaks of the open records and of their bytes (the definition's table: pool and
    window), windows the device handed to the host form for a run of equal hashes.  All zero after a call that did not collate."""
    L = load_library()
    L.bmh_reads_last_collate_counts.argtypes = [C.POINTER(CollateCountsT)]
    c = CollateCountsT()
    L.bmh_reads_last_collate_counts(C.byref(c))
    return {n: int(getattr(c, n)) for n, _t in CollateCountsT._fields_}


READS_KEEP_RG = 8           # BMH_READS_KEEP_RG


def _collate_cap(collate, collate_mem) -> int:
    """collate_mem as bmh_reads_load_files_ex / bmh_bam_reads_ex take it (0: the default cap)"""
    if collate_mem is not None and not collate:
        raise ValueError("collate_mem without collate=True: the cap is that of the collation's open records")
    if collate_mem is not None and int(collate_mem) < 1:
        raise ValueError("collate_mem: a number of bytes, 1 or more")
    return int(collate_mem or 0)


def reads_last_counts() -> dict:
    """bmh_reads_last_counts: how the last load_reads_files / run_files call of the process cut its text -- windows on the device, windows the host walked
    (the fallback), text bytes, records"""
    L = load_library()
    L.bmh_reads_last_counts.argtypes = [C.POINTER(C.c_uint64)]
    out = (C.c_uint64 * 4)()
    L.bmh_reads_last_counts(out)
    L.bmh_reads_last_inflate_counts.argtypes = [C.POINTER(C.c_uint64)]
    inf = (C.c_uint64 * 2)()
    L.bmh_reads_last_inflate_counts(inf)
    return dict(device_windows=int(out[0]), host_windows=int(out[1]), text_bytes=int(out[2]), records=int(out[3]),
                device_inflate_members=int(inf[0]), host_inflate_members=int(inf[1]))


def reseed_last_counts() -> dict:
    """bmh_reseed_last_counts: the path the calling thread's last bmh_seed_batch_reseed took -- round-2 tasks, tasks that overflowed the first launch's
    column (knob RESEED_CAP), seed groups of rounds 1, 2 and 3, rank steps of round 2 (both launches) and of round 3"""
    out = (C.c_uint64 * 7)()
    L = load_library()
    if L.bmh_reseed_last_counts(out) != 0:
        raise RuntimeError("bmh_reseed_last_counts: " + _err(L))
    return dict(tasks=int(out[0]), overflowed=int(out[1]), rounds=(int(out[2]), int(out[3]), int(out[4])), steps=(int(out[5]), int(out[6])))


# ---- BGZF members inflated on the device (csrc/inflate_kernels.hip) or by the same decoder on the host
INFLATE_HOST = 1            # BMH_INFLATE_HOST
INFLATE_MEMBER = np.dtype([("in_off", "<u8"), ("out_off", "<u8"), ("in_len", "<u4"), ("isize", "<u4"), ("crc32", "<u4"), ("reserved", "<u4")])     # bmh_inflate_member_t
INFLATE_STATUS = ("ok", "block_type", "stored_len", "code_lengths", "symbol", "distance", "truncated", "size", "crc", "table")


def bgzf_scan(data: bytes) -> tuple:
    """bmh_bgzf_scan: (member table as an INFLATE_MEMBER array, bytes the whole members cover, bytes of text).  Bytes that begin no BGZF member raise ValueError;
    a cut last member is left out (used < len(data))."""
    L = load_library()
    L.bmh_bgzf_scan.argtypes = [C.c_char_p, C.c_uint64, C.c_void_p, C.c_uint64, _u64p, _u64p, _u64p]
    nm, used, text = C.c_uint64(), C.c_uint64(), C.c_uint64()
    if L.bmh_bgzf_scan(data, len(data), None, 0, C.byref(nm), C.byref(used), C.byref(text)) != 0:
        raise ValueError(_err(L))
    tab = np.zeros(int(nm.value), INFLATE_MEMBER)
    if L.bmh_bgzf_scan(data, len(data), tab.ctypes.data if len(tab) else None, len(tab), C.byref(nm), C.byref(used), C.byref(text)) != 0:
        raise ValueError(_err(L))
    return tab, int(used.value), int(text.value)


def inflate_members(data: bytes, tab: np.ndarray, out_bytes: int, host: bool = False, per_launch: int = 0) -> tuple:
    """bmh_inflate_members_device (or _host): the members of `tab` (INFLATE_MEMBER, offsets into data and into the text) -> (text as a uint8 array, status per
    member); per_launch > 0: that many members per kernel launch"""
    L = load_library()
    tab = np.ascontiguousarray(tab, INFLATE_MEMBER)
    n = len(tab)
    if host:
        out, st = np.zeros(out_bytes + 1, np.uint8), np.zeros(n, np.uint32)
        L.bmh_inflate_members_host.argtypes = [C.c_char_p, C.c_uint64, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint64, C.c_void_p, C.c_int]
        if L.bmh_inflate_members_host(data, len(data), tab.ctypes.data, n, out.ctypes.data, out_bytes, st.ctypes.data, 0) != 0:
            raise RuntimeError("bmh_inflate_members_host: " + _err(L))
        return out[:out_bytes], st
    import torch
    d_in = torch.from_numpy(np.frombuffer(data + b"\0", np.uint8).copy()).cuda()
    d_tab = torch.from_numpy(tab.view(np.uint8).reshape(-1).copy() if n else np.zeros(1, np.uint8)).cuda()
    d_out = torch.zeros(out_bytes + 1, dtype=torch.uint8, device="cuda")
    d_st = torch.full((max(n, 1),), 0x7fffffff, dtype=torch.int32, device="cuda")
    L.bmh_inflate_members_device.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p]
    step = per_launch if per_launch > 0 else max(n, 1)
    stream = torch.cuda.current_stream().cuda_stream
    for a in range(0, n, step):
        k = min(step, n - a)
        if L.bmh_inflate_members_device(d_in.data_ptr(), len(data), d_tab.data_ptr() + a * INFLATE_MEMBER.itemsize, k, d_out.data_ptr(), out_bytes,
                                        d_st.data_ptr() + 4 * a, stream) != 0:
            raise RuntimeError("bmh_inflate_members_device: " + _err(L))
    torch.cuda.synchronize()
    return d_out.cpu().numpy()[:out_bytes], d_st.cpu().numpy()[:n].astype(np.uint32)


def inflate_bgzf(data: bytes, host: bool = False) -> bytes:
    """bmh_bgzf_inflate: the text of a BGZF file held in memory, inflated on the device -- host=True: by the same decoder as plain C++, no device needed.
    A cut file, bytes that are no BGZF member or a damaged member (inflate, length or CRC32) raise ValueError."""
    L = load_library()
    L.bmh_bgzf_inflate.argtypes = [C.c_char_p, C.c_uint64, C.c_int, C.POINTER(C.c_void_p), _u64p]
    L.bmh_free.argtypes = [C.c_void_p]
    text, n = C.c_void_p(), C.c_uint64()
    rc = L.bmh_bgzf_inflate(data, len(data), INFLATE_HOST if host else 0, C.byref(text), C.byref(n))
    if rc != 0:
        msg = _err(L)
        raise ValueError(msg) if rc == -2 else RuntimeError("bmh_bgzf_inflate: " + msg)
    try:
        return C.string_at(text.value, n.value)
    finally:
        L.bmh_free(text)


# ---- BAM output: SAM record lines -> BAM records -> BGZF members (csrc/bam_kernels.hip, csrc/deflate_kernels.hip), or the same cores on the host
OUT_SAM, OUT_BAM = 0, 1     # BMH_OUT_SAM, BMH_OUT_BAM
BAM_STATUS = ("ok", "fields", "name", "cigar", "tag", "seq_qual", "no_eol", "rname", "number", "int_tag", "float_tag", "b_array", "size")


class BamOut(C.Structure):
    """bmh_bam_out_t"""
    _fields_ = [("d_bam", C.c_void_p), ("bam_bytes", C.c_uint64), ("d_status", C.c_void_p), ("n_records", C.c_uint32),
                ("n_refused", C.c_uint32), ("first_refused", C.c_uint32), ("first_status", C.c_uint32)]


class BamRefusal(ValueError):
    """a SAM record that cannot be written as BAM (the message names the read and the check)"""


def _contig_table(contigs) -> tuple:
    """names NUL-terminated back to back, offsets [n + 1]; contigs: names, or (name, length) pairs"""
    names = [(c if isinstance(c, (str, bytes)) else c[0]) for c in contigs]
    names = [n.encode() if isinstance(n, str) else bytes(n) for n in names]
    off = np.zeros(len(names) + 1, np.uint32)
    off[1:] = np.cumsum([len(n) + 1 for n in names], dtype=np.int64)
    return np.frombuffer(b"".join(n + b"\0" for n in names) + b"\0", np.uint8).copy(), off


def bgzf_eof() -> bytes:
    """bmh_bgzf_eof: the 28-byte end-of-file member"""
    return bytes((C.c_uint8 * 28).in_dll(load_library(), "bmh_bgzf_eof"))


def bam_status_name(status: int) -> str:
    L = load_library()
    L.bmh_bam_status_name.restype = C.c_char_p
    L.bmh_bam_status_name.argtypes = [C.c_uint32]
    return L.bmh_bam_status_name(int(status)).decode()


def sam_to_bam(text: bytes, contigs, host: bool = False) -> tuple:
    """bmh_sam_to_bam_device (host=True: bmh_sam_to_bam_host, no device needed): SAM record lines -> (the BAM records back to back as bytes, status per
    line as a uint32 array: 0, or the index into BAM_STATUS of the check that refused the line, which then left no bytes)"""
    L = load_library()
    text = bytes(text)
    blob, off = _contig_table(contigs)
    nc = len(off) - 1
    if host:
        L.bmh_sam_to_bam_host.argtypes = [C.c_char_p, C.c_uint64, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.POINTER(C.c_void_p), _u64p, C.POINTER(C.c_void_p), _u32p]
        L.bmh_free.argtypes = [C.c_void_p]
        bam, st, nb, nr = C.c_void_p(), C.c_void_p(), C.c_uint64(), C.c_uint32()
        if L.bmh_sam_to_bam_host(text, len(text), nc, blob.ctypes.data, off.ctypes.data, 0, C.byref(bam), C.byref(nb), C.byref(st), C.byref(nr)) != 0:
            raise RuntimeError("bmh_sam_to_bam_host: " + _err(L))
        try:
            return C.string_at(bam.value, nb.value) if nb.value else b"", np.frombuffer(C.string_at(st.value, 4 * nr.value), np.uint32).copy()
        finally:
            L.bmh_free(bam); L.bmh_free(st)
    import torch
    L.bmh_bam_ws_create.restype = C.c_void_p
    L.bmh_bam_ws_free.argtypes = [C.c_void_p]
    L.bmh_sam_to_bam_device.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(BamOut)]
    d_text = torch.from_numpy(np.frombuffer(text + b"\0", np.uint8).copy()).cuda()
    d_blob, d_off = torch.from_numpy(blob).cuda(), torch.from_numpy(off.view(np.int32).copy()).cuda()
    ws = L.bmh_bam_ws_create()
    try:
        o = BamOut()
        if L.bmh_sam_to_bam_device(ws, d_text.data_ptr(), len(text), nc, d_blob.data_ptr(), d_off.data_ptr(), torch.cuda.current_stream().cuda_stream, C.byref(o)) != 0:
            raise RuntimeError("bmh_sam_to_bam_device: " + _err(L))
        bam = torch.empty(max(int(o.bam_bytes), 1), dtype=torch.uint8, device="cuda"); st = torch.empty(max(int(o.n_records), 1), dtype=torch.int32, device="cuda")
        if o.bam_bytes: _memcpy_d2d(bam.data_ptr(), o.d_bam, int(o.bam_bytes))
        if o.n_records: _memcpy_d2d(st.data_ptr(), o.d_status, 4 * int(o.n_records))
        torch.cuda.synchronize()
        return bam.cpu().numpy()[:int(o.bam_bytes)].tobytes(), st.cpu().numpy()[:int(o.n_records)].view(np.uint32).copy()
    finally:
        L.bmh_bam_ws_free(ws)


def bgzf_compress(data: bytes, level: int = 1, host: bool = False) -> bytes:
    """bmh_bgzf_deflate_device (host=True: bmh_bgzf_deflate_host): the bytes as BGZF members of at most 0xff00 bytes of data each (level 0: stored, 1: LZ77 +
    dynamic Huffman codes); no bytes give no members.  Both forms give the same bytes.  The caller appends bgzf_eof() to end a file."""
    L = load_library()
    data = bytes(data)
    if host:
        L.bmh_bgzf_deflate_host.argtypes = [C.c_char_p, C.c_uint64, C.c_int, C.c_int, C.POINTER(C.c_void_p), _u64p]
        L.bmh_free.argtypes = [C.c_void_p]
        out, n = C.c_void_p(), C.c_uint64()
        if L.bmh_bgzf_deflate_host(data, len(data), int(level), 0, C.byref(out), C.byref(n)) != 0:
            raise ValueError("bmh_bgzf_deflate_host: " + _err(L))
        try:
            return C.string_at(out.value, n.value) if n.value else b""
        finally:
            L.bmh_free(out)
    import torch
    L.bmh_bam_ws_create.restype = C.c_void_p
    L.bmh_bam_ws_free.argtypes = [C.c_void_p]
    L.bmh_bgzf_deflate_device.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_int, C.c_void_p, C.POINTER(C.c_void_p), _u64p]
    d_in = torch.from_numpy(np.frombuffer(data + b"\0", np.uint8).copy()).cuda()
    ws = L.bmh_bam_ws_create()
    try:
        out, n = C.c_void_p(), C.c_uint64()
        if L.bmh_bgzf_deflate_device(ws, d_in.data_ptr(), len(data), int(level), torch.cuda.current_stream().cuda_stream, C.byref(out), C.byref(n)) != 0:
            raise ValueError("bmh_bgzf_deflate_device: " + _err(L))
        if not n.value:
            return b""
        t = torch.empty(int(n.value), dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        _memcpy_d2d(t.data_ptr(), out.value, int(n.value))
        torch.cuda.synchronize()
        return t.cpu().numpy().tobytes()
    finally:
        L.bmh_bam_ws_free(ws)


def bam_header(header_text: str, contigs) -> bytes:
    """bmh_bam_header: magic, l_text, text, n_ref and the references of (name, length) pairs -- uncompressed"""
    L = load_library()
    L.bmh_bam_header.argtypes = [C.c_char_p, C.c_int, C.POINTER(C.c_char_p), C.c_void_p, C.POINTER(C.c_void_p), _u64p]
    L.bmh_free.argtypes = [C.c_void_p]
    names = (C.c_char_p * max(len(contigs), 1))(*[c[0].encode() for c in contigs])
    lens = np.ascontiguousarray([c[1] for c in contigs] or [0], dtype=np.int32)
    out, n = C.c_void_p(), C.c_uint64()
    if L.bmh_bam_header(header_text.encode(), len(contigs), names, lens.ctypes.data, C.byref(out), C.byref(n)) != 0:
        raise ValueError("bmh_bam_header: " + _err(L))
    try:
        return C.string_at(out.value, n.value)
    finally:
        L.bmh_free(out)


# ---- coordinate-sorted BAM and its BAI index (csrc/bam_sort_core.h, csrc/bam_sort_kernels.hip, csrc/bam_sort_host.cpp)
OUT_BAM_SORTED = 2          # BMH_OUT_BAM_SORTED


def bam_sort(records: bytes, host: bool = False) -> bytes:
    """bmh_bam_sort_device (host=True: bmh_bam_sort_host, std::stable_sort, no device needed): a stream of BAM records in coordinate order -- `samtools sort`'s
    key, equal keys in the order they came in.  A stream that is not a whole number of records raises ValueError."""
    L = load_library()
    records = bytes(records)
    L.bmh_free.argtypes = [C.c_void_p]
    out = C.c_void_p()
    if host:
        L.bmh_bam_sort_host.argtypes = [C.c_char_p, C.c_uint64, C.POINTER(C.c_void_p)]
        rc = L.bmh_bam_sort_host(records, len(records), C.byref(out))
    else:
        import torch
        L.bmh_bam_sort_device.argtypes = [C.c_char_p, C.c_uint64, C.c_void_p, C.POINTER(C.c_void_p)]
        rc = L.bmh_bam_sort_device(records, len(records), torch.cuda.current_stream().cuda_stream, C.byref(out))
    if rc != 0:
        raise (ValueError if rc == -2 else RuntimeError)("bmh_bam_sort: " + _err(L))
    try:
        return C.string_at(out.value, len(records)) if records else b""
    finally:
        L.bmh_free(out)


# ---- duplicate marking (csrc/bam_dup_core.h, csrc/bam_dup_kernels.hip, csrc/bam_dup_host.cpp)
MARKDUP_COUNTS = ("pairs_examined", "fragments_examined", "duplicate_pairs", "duplicate_fragments", "records_flagged", "secondary_or_supplementary", "unmapped_records", "templates")


def _library_table(read_groups):
    """[(id, library_name), ...] -> (the C arrays of the _groups entry points: ids, library indices, their count; the library names in order of first appearance).
    Groups with one library name are lanes of one library; the indices are not checked here (the library refuses more than 255 and repeated IDs by row)"""
    names = []
    for _rid, lb in read_groups:
        if lb not in names:
            names.append(lb)
    ids = (C.c_char_p * max(len(read_groups), 1))(*[(rid if isinstance(rid, bytes) else str(rid).encode()) for rid, _lb in read_groups])
    lib = (C.c_int32 * max(len(read_groups), 1))(*[names.index(lb) for _rid, lb in read_groups])
    return ids, lib, len(read_groups), names


def _library_counts(names, flat) -> dict:
    return {nm: dict(zip(MARKDUP_COUNTS, (int(v) for v in flat[8 * k:8 * k + 8]))) for k, nm in enumerate(names)}


OPTICAL_COUNTS = ("optical_duplicate_pairs", "located_pairs", "optical_sets_skipped")
LOCATION_DTYPE = np.dtype([("x", "<i4"), ("y", "<i4"), ("tile", "<u4"), ("rg", "<u2"), ("flags", "<u2")])      # bdp_loc_t; flags: 1 located, 2 role


def optical_distance_value(value, what: str) -> int:
    """the keyword optical_distance of the marking calls: an integer in 0 .. 2^31 - 1; ValueError otherwise"""
    if not isinstance(value, (int, np.integer)) or isinstance(value, bool) or not 0 <= value <= 0x7fffffff:
        raise ValueError(f"{what}: optical_distance {value!r}: an integer in 0 .. 2^31 - 1")
    return int(value)


BARCODE_OFF, BARCODE_TAG, BARCODE_NAME = 0, 1, 2
_OWN_TAGS = ("RG", "NM", "MD", "AS", "XS", "SA", "XA", "pa")


def barcode_source(barcode_tag, barcode_name, what: str) -> tuple:
    """the keywords barcode_tag ("RX": a tag of type Z on a template's first record) and barcode_name (True: the read name's last ':' field) of the marking calls
    -> (mode, tag bytes) for the C entry points; (0, None) when neither is given.  ValueError: both at once, a tag that is not [A-Za-z][A-Za-z0-9], RG, or a tag
    the aligner writes itself (NM MD AS XS SA XA pa)"""
    if barcode_name is not None and not isinstance(barcode_name, (bool, np.bool_)):
        raise ValueError(f"{what}: barcode_name {barcode_name!r}: True or False")
    if barcode_tag is not None and barcode_name:
        raise ValueError(f"{what}: barcode_tag and barcode_name are two sources of one barcode: give one")
    if barcode_tag is None:
        return (BARCODE_NAME, None) if barcode_name else (BARCODE_OFF, None)
    tag = barcode_tag.decode("latin-1") if isinstance(barcode_tag, bytes) else barcode_tag
    if not isinstance(tag, str) or len(tag) != 2 or not (tag[0].isascii() and tag[0].isalpha() and tag[1].isascii() and tag[1].isalnum()):
        raise ValueError(f"{what}: barcode_tag {barcode_tag!r}: two characters, [A-Za-z][A-Za-z0-9]")
    if tag in _OWN_TAGS:
        raise ValueError(f"{what}: barcode_tag {tag}: RG names the read group, and NM MD AS XS SA XA pa are written by the aligner itself")
    return BARCODE_TAG, tag.encode()


BARCODE_GROUP_COUNTS = ("pair_barcodes_observed", "pair_barcodes_inferred", "barcode_keys_skipped")
BARCODE_MAX_EDITS = 21


def barcode_edits_value(barcode_edits, bc_mode, what: str) -> int:
    """the keyword barcode_edits (None: barcodes are compared exactly; N: barcodes within N mismatches are one molecule) of the marking calls -> the C entry
    points' edits (-1: off).  ValueError: not an integer in 0 .. 21, or no barcode source beside it"""
    if barcode_edits is None:
        return -1
    if not isinstance(barcode_edits, (int, np.integer)) or isinstance(barcode_edits, (bool, np.bool_)) or not 0 <= barcode_edits <= BARCODE_MAX_EDITS:
        raise ValueError(f"{what}: barcode_edits {barcode_edits!r}: an integer in 0 .. {BARCODE_MAX_EDITS}")
    if bc_mode == BARCODE_OFF:
        raise ValueError(f"{what}: barcode_edits groups the barcodes that are compared: it needs barcode_tag or barcode_name")
    return int(barcode_edits)


def barcode_pack(value) -> int:
    """bmh_barcode_pack: the packed word duplicate marking compares for a barcode value (bytes or str) when barcodes are grouped by edits -- 3 bits a byte (A 1, C 2,
    G 3, T 4, N 5, - 6, + 7), symbol i in bits 3 i .. 3 i + 2, 0 for the empty value (no barcode).  ValueError: more than 21 bytes, or a byte without a symbol"""
    L = load_library()
    value = value if isinstance(value, bytes) else str(value).encode()
    w = C.c_uint64(0)
    L.bmh_barcode_pack.argtypes = [C.c_char_p, C.c_uint64, C.POINTER(C.c_uint64)]
    if L.bmh_barcode_pack(value, len(value), C.byref(w)) != 1:
        raise ValueError(f"barcode_pack: {value!r} does not pack: at most 21 bytes of A C G T N - +")
    return int(w.value)


def barcode_word(value) -> int:
    """bmh_barcode_word: the 64-bit word duplicate marking compares for a barcode value (bytes or str) -- FNV-1a, 0 for the empty value (no barcode), 1 for a
    value that hashes to 0"""
    L = load_library()
    value = value if isinstance(value, bytes) else str(value).encode()
    L.bmh_barcode_word.argtypes = [C.c_char_p, C.c_uint64]
    L.bmh_barcode_word.restype = C.c_uint64
    return int(L.bmh_barcode_word(value, len(value)))


def bam_dup_barcodes(records: bytes, host: bool = False, tag=None, name=None, edits: bool = False) -> np.ndarray:
    """bmh_bam_dup_barcodes_device (host=True: _host): a record stream as bam_markdup takes it -> one barcode word (uint64) per template, from tag `tag` of its first
    record or (name=True) from its read name's last ':' field; 0: no barcode.  This is what bam_markdup(barcode_tag=...) compares.
    edits=True (packed = 1): the packed words (barcode_pack) that bam_markdup(barcode_edits=...) groups; a value that does not pack raises
    ValueError with its record's index."""
    mode, tg = barcode_source(tag, name, "bam_dup_barcodes")
    if mode == BARCODE_OFF:
        raise ValueError("bam_dup_barcodes: give tag= or name=True")
    L = load_library()
    records = bytes(records)
    L.bmh_free.argtypes = [C.c_void_p]
    out, nt = C.c_void_p(), C.c_uint64(0)
    head = [C.c_char_p, C.c_uint64, C.c_int, C.c_char_p, C.c_int]
    if host:
        L.bmh_bam_dup_barcodes_host.argtypes = head + [C.POINTER(C.c_void_p), C.POINTER(C.c_uint64)]
        rc = L.bmh_bam_dup_barcodes_host(records, len(records), mode, tg, 1 if edits else 0, C.byref(out), C.byref(nt))
    else:
        import torch
        L.bmh_bam_dup_barcodes_device.argtypes = head + [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_uint64)]
        rc = L.bmh_bam_dup_barcodes_device(records, len(records), mode, tg, 1 if edits else 0, torch.cuda.current_stream().cuda_stream, C.byref(out), C.byref(nt))
    if rc != 0:
        raise (ValueError if rc == -2 else RuntimeError)("bmh_bam_dup_barcodes: " + _err(L))
    try:
        return np.frombuffer(C.string_at(out.value, 8 * nt.value) if nt.value else b"", dtype="<u8").copy()
    finally:
        L.bmh_free(out)


class MarkdupOpt(C.Structure):
    """bmh_markdup_opt_t"""
    _fields_ = [("rg_ids", C.POINTER(C.c_char_p)), ("rg_lib", C.POINTER(C.c_int32)), ("n_groups", C.c_int32), ("optical_distance", C.c_int64), ("optical_max_set", C.c_uint64),
                ("barcode_mode", C.c_int32), ("barcode_tag", C.c_char * 2), ("barcode_edits", C.c_int32), ("barcode_max_set", C.c_uint64)]


class MarkdupCounts(C.Structure):
    """bmh_markdup_counts_t"""
    _fields_ = [("counts", C.c_uint64 * 8), ("optical", C.c_uint64 * 3), ("grouped", C.c_uint64 * 3), ("no_barcode", C.c_uint64),
                ("lib_counts", _u64p), ("lib_optical", _u64p), ("lib_grouped", _u64p)]


def _markdup_api(L):
    """the library with the argument types of the two calls that take the records above"""
    if not getattr(L, "_markdup_api", False):
        stream, out = [C.c_char_p, C.c_uint64, C.POINTER(MarkdupOpt)], [C.POINTER(C.c_void_p), C.POINTER(MarkdupCounts)]
        L.bmh_markdup_opt_default.argtypes, L.bmh_markdup_opt_default.restype = [C.POINTER(MarkdupOpt)], None
        L.bmh_bam_markdup_host.argtypes, L.bmh_bam_markdup_device.argtypes = stream + out, stream + [C.c_void_p] + out
        L.bmh_free.argtypes = [C.c_void_p]
        L._markdup_api = True
    return L


def _markdup_records(L, read_groups, distance=-1, max_set=0, bc_mode=BARCODE_OFF, bc_tag=None, edits=-1, bc_max_set=0) -> tuple:
    """the validated keywords of the marking calls -> (bmh_markdup_opt_t, bmh_markdup_counts_t with a library's arrays where read_groups are given, the library
    names, what the records point into: kept by the caller until the call is over)"""
    o, res = MarkdupOpt(), MarkdupCounts()
    L.bmh_markdup_opt_default(C.byref(o))
    o.optical_distance, o.optical_max_set, o.barcode_mode, o.barcode_edits, o.barcode_max_set = distance, max_set, bc_mode, edits, bc_max_set
    if bc_tag is not None:
        o.barcode_tag = bc_tag
    names, keep = [], []
    if read_groups is not None:
        ids, lib, o.n_groups, names = _library_table(read_groups)
        o.rg_ids, o.rg_lib = ids, lib
        arrays = [(C.c_uint64 * (k * max(len(names), 1)))() for k in (8, 3, 3)]
        res.lib_counts, res.lib_optical, res.lib_grouped = (C.cast(a, _u64p) for a in arrays)
        keep = [ids, lib] + arrays
    return o, res, names, keep


def _markdup_dict(o, res, names, with_libraries: bool) -> dict:
    """the counts of a marking call by the names of MARKDUP_COUNTS, OPTICAL_COUNTS (with an optical distance), "templates_without_barcode" (with a barcode source),
    BARCODE_GROUP_COUNTS (with edits) and "libraries" (with read groups)"""
    optical, barcode = o.optical_distance >= 0, o.barcode_mode != BARCODE_OFF
    grouped = barcode and o.barcode_edits >= 0
    c = dict(zip(MARKDUP_COUNTS, (int(v) for v in res.counts)))
    if optical:
        c.update(zip(OPTICAL_COUNTS, (int(v) for v in res.optical)))
    if barcode:
        c["templates_without_barcode"] = int(res.no_barcode)
    if grouped:
        c.update(zip(BARCODE_GROUP_COUNTS, (int(v) for v in res.grouped)))
    if with_libraries:
        c["libraries"] = _library_counts(names, res.lib_counts)
        for k, nm in enumerate(names):
            if optical:
                c["libraries"][nm].update(zip(OPTICAL_COUNTS, (int(v) for v in res.lib_optical[3 * k:3 * k + 3])))
            if grouped:
                c["libraries"][nm].update(zip(BARCODE_GROUP_COUNTS, (int(v) for v in res.lib_grouped[3 * k:3 * k + 3])))
    return c


def bam_dup_locations(records: bytes, host: bool = False, read_groups=None) -> np.ndarray:
    """bmh_bam_dup_locations_device (host=True: _host): a record stream as bam_markdup takes it -> one location per template, a structured array of LOCATION_DTYPE
    (x, y, tile, rg: the row of the template's read group in read_groups, 0 without them; flags: 1 located, 2 role).  This is the optical step's first half on its own."""
    L = load_library()
    records = bytes(records)
    L.bmh_free.argtypes = [C.c_void_p]
    out, nt = C.c_void_p(), C.c_uint64(0)
    ids = lib = None
    ng = 0
    if read_groups is not None:
        ids, lib, ng, _names = _library_table(read_groups)
    head = [C.c_char_p, C.c_uint64, C.POINTER(C.c_char_p), C.POINTER(C.c_int32), C.c_int]
    if host:
        L.bmh_bam_dup_locations_host.argtypes = head + [C.POINTER(C.c_void_p), C.POINTER(C.c_uint64)]
        rc = L.bmh_bam_dup_locations_host(records, len(records), ids, lib, ng, C.byref(out), C.byref(nt))
    else:
        import torch
        L.bmh_bam_dup_locations_device.argtypes = head + [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_uint64)]
        rc = L.bmh_bam_dup_locations_device(records, len(records), ids, lib, ng, torch.cuda.current_stream().cuda_stream, C.byref(out), C.byref(nt))
    if rc != 0:
        raise (ValueError if rc == -2 else RuntimeError)("bmh_bam_dup_locations: " + _err(L))
    try:
        return np.frombuffer(C.string_at(out.value, 16 * nt.value) if nt.value else b"", dtype=LOCATION_DTYPE).copy()
    finally:
        L.bmh_free(out)


def bam_name_location(name):
    """bmh_bam_name_location: the read name's (tile, x, y) by the optical step's rules, or None when it has no location"""
    L = load_library()
    name = name if isinstance(name, bytes) else str(name).encode()
    out = (C.c_uint32 * 3)()
    L.bmh_bam_name_location.argtypes = [C.c_char_p, C.c_uint32, C.POINTER(C.c_uint32)]
    rc = L.bmh_bam_name_location(name, len(name), out)
    if rc < 0:
        raise ValueError("bmh_bam_name_location: " + _err(L))
    return (int(out[0]), int(out[1]), int(out[2])) if rc == 1 else None


def estimate_library_size(n: int, c: int):
    """bmh_library_size: Picard's ESTIMATED_LIBRARY_SIZE from n = pairs examined minus optical duplicate pairs and c = pairs examined minus duplicate pairs; None
    where Picard leaves the column empty (n == 0 or nothing duplicated)"""
    L = load_library()
    if n < 0 or c < 0:
        return None
    size = C.c_int64(0)
    L.bmh_library_size.argtypes = [C.c_uint64, C.c_uint64, C.POINTER(C.c_int64)]
    return int(size.value) if L.bmh_library_size(int(n), int(c), C.byref(size)) == 1 else None


def bam_markdup(records: bytes, host: bool = False, read_groups=None, optical_distance=None, optical_max_set=None, barcode_tag=None, barcode_name=None, barcode_edits=None,
                barcode_max_set=None) -> tuple:
    """bmh_bam_markdup_device (host=True: bmh_bam_markdup_host, no device needed) under one bmh_markdup_opt_t: a stream of BAM records in the writer's order (a template's records next to
    each other, its first primary line first) -> (the same records with flag 0x400 on every record of every duplicate template, the counts by MARKDUP_COUNTS'
    names).  Picard MarkDuplicates' rules.  A cut stream, one whose first record begins no template and a paired template without both of its
    primary lines raise ValueError.
    read_groups: [(id, library_name), ...] (rg_ids, rg_lib, n_groups) -- duplicates are called within a library only, a template's library being that of the RG:Z
    tag on its first record; the counts gain "libraries": {library_name: counts}, in order of first appearance.  A template without the tag or with an ID that is
    not listed, more than 255 libraries and a repeated ID raise ValueError.  Without read_groups no tag is read.
    optical_distance (optical_distance, optical_max_set): also count the optical duplicates -- pairs of one duplicate set whose names place them on one tile within that
    many pixels in x and y -- the counts gain OPTICAL_COUNTS' names, with read_groups per library too; the records are those of the call without
    it.  optical_max_set (needs optical_distance; default 300 000): sets of more pairs are not examined.
    barcode_tag="RX" or barcode_name=True (barcode_mode, barcode_tag; one of the two): templates with different molecular barcodes (UMIs) are no duplicates of each
    other -- the barcode is the value of that tag (type Z, verbatim) on the template's first record, or the read name's last ':' field; the keys become (lo, hi,
    barcode) and (end, barcode), an optical set the pairs of one (lo, hi, barcode).  Templates without a barcode are comparable with each other only; the counts gain
    "templates_without_barcode".  A first record whose tag has another type, or whose tags cannot be walked, raises ValueError with its index.
    barcode_edits=N (barcode_edits, barcode_max_set; 0 .. 21, beside a barcode source): barcodes within N mismatches are one molecule -- within one
    (library, lo, hi) the pairs' distinct barcodes are clustered transitively and compared by their cluster's smallest, and likewise, on their own, the barcodes at
    one (library, end) before the fragment rule.  Barcodes are packed (barcode_pack): a value of more than 21 bytes or with a byte other than A C G T N - + raises
    ValueError with its record's index.  The counts gain BARCODE_GROUP_COUNTS' names, with read_groups per library too.  barcode_max_set (needs barcode_edits; default
    65 536; for tests): a key with more distinct barcodes is not clustered."""
    L = _markdup_api(load_library())
    records = bytes(records)
    if optical_max_set is not None and optical_distance is None:
        raise ValueError("bam_markdup: optical_max_set needs optical_distance")
    bc_mode, bc_tag = barcode_source(barcode_tag, barcode_name, "bam_markdup")
    edits = barcode_edits_value(barcode_edits, bc_mode, "bam_markdup")
    if barcode_max_set is not None and edits < 0:
        raise ValueError("bam_markdup: barcode_max_set needs barcode_edits")
    if barcode_max_set is not None and (not isinstance(barcode_max_set, (int, np.integer)) or isinstance(barcode_max_set, bool) or not 1 <= barcode_max_set <= 0x7fffffff):
        raise ValueError(f"bam_markdup: barcode_max_set {barcode_max_set!r}: an integer in 1 .. 2^31 - 1")
    distance = -1 if optical_distance is None else optical_distance_value(optical_distance, "bam_markdup")
    if optical_max_set is not None and (not isinstance(optical_max_set, (int, np.integer)) or isinstance(optical_max_set, bool) or not 1 <= optical_max_set <= 0x7fffffff):
        raise ValueError(f"bam_markdup: optical_max_set {optical_max_set!r}: an integer in 1 .. 2^31 - 1")
    o, res, names, _keep = _markdup_records(L, read_groups, distance, int(optical_max_set or 0), bc_mode, bc_tag, edits, int(barcode_max_set or 0))
    out = C.c_void_p()
    if host:
        rc = L.bmh_bam_markdup_host(records, len(records), C.byref(o), C.byref(out), C.byref(res))
    else:
        import torch
        rc = L.bmh_bam_markdup_device(records, len(records), C.byref(o), torch.cuda.current_stream().cuda_stream, C.byref(out), C.byref(res))
    if rc != 0:
        raise (ValueError if rc == -2 else RuntimeError)("bmh_bam_markdup: " + _err(L))
    try:
        return (C.string_at(out.value, len(records)) if records else b""), _markdup_dict(o, res, names, read_groups is not None)
    finally:
        L.bmh_free(out)


INDEX_BAI, INDEX_CSI = 0, 1


def index_format_code(index_format, csi_min_shift, what: str) -> tuple:
    """the keywords index_format ("bai" or "csi") and csi_min_shift (10 .. 24, with "csi" only) of the sorting calls -> (BMH_INDEX_*, min_shift); ValueError otherwise"""
    if index_format not in ("bai", "csi"):
        raise ValueError(f"{what}: index_format {index_format!r}: bai or csi")
    if not isinstance(csi_min_shift, (int, np.integer)) or isinstance(csi_min_shift, bool):
        raise ValueError(f"{what}: csi_min_shift {csi_min_shift!r}: an integer in 10 .. 24")
    if index_format != "csi":
        if csi_min_shift != 14:
            raise ValueError(f'{what}: csi_min_shift={csi_min_shift} needs index_format="csi" (a BAI index has no other than 14)')
        return INDEX_BAI, 14
    if not 10 <= csi_min_shift <= 24:
        raise ValueError(f"{what}: csi_min_shift {csi_min_shift}: a CSI index takes 10 .. 24 (14 is BAI's)")
    return INDEX_CSI, int(csi_min_shift)


def bam_sorted_file(header_text: str, contigs, records: bytes, level: int = 1, window: int = 0, host: bool = False, markdup: bool = False, read_groups=None,
                    index_format: str = "bai", csi_min_shift: int = 14, barcode_tag=None, barcode_name=None, barcode_edits=None, coverage=None, stats=None,
                    optical_distance=None, recal=None, apply_recal=None, apply_recal_report=None) -> tuple:
    """apply_recal (a path or read_recal_table's dict): the qualities of every record are recalibrated by that table as the windows are written;
    the tuple's last element is then the recal dict with the step's counts under "apply" (alone there when recal is None), and apply_recal_report (a path or a
    text file object) takes recal_apply_report_text's rows.
    recal={pac, l_pac, contig_offset, mask, read_groups, min_qual, max_cycle, known_sites} (bmh_sorted_opt_t's recal; recal_opt's keywords): the file's covariate
    table (bam_recal's dict), from the same windows with the flags markdup=True sets, comes last in the tuple.
    stats={insert_cap} (bmh_sorted_opt_t's stats; {} for the default): the file's statistics (bam_stats' dict), taken from the same windows with the flags
    markdup=True sets, come last in the tuple, behind the coverage where both are asked for.
    coverage={min_mapq, deletions, bin, tile} (bmh_sorted_opt_t's coverage; bam_coverage's keywords, {} for the defaults): the file's coverage, taken from
    the windows of the merge as they are written -- with markdup=True the marked duplicates are counted out -- comes last in the tuple.
    bmh_bam_sorted_file_device (host=True: _host): (the complete sorted BAM file -- header members, the records in coordinate order in windows of `window`
    records (0: about 64 MiB), the end-of-file member --, its .bai index).  contigs: (name, length) pairs; both forms give the same bytes.
    markdup=True (a bmh_markdup_opt_t in bmh_sorted_opt_t): `records` come in the writer's order, the duplicates among them are marked (bam_markdup's rules) and the counts come third.
    read_groups (needs markdup=True): as bam_markdup takes them -- duplicates per library, and the counts gain "libraries".
    index_format="csi" (index_format, min_shift): the second element is the .csi index -- BGZF-compressed, bins of 2^csi_min_shift bases (10 .. 24) at the depth the
    longest contig asks for --, contigs may hold up to 2^31 - 1 bases (with markdup=True up to 2^30 - 2^24) and the BAM bytes are those of the "bai" call.
    barcode_tag / barcode_name (need markdup=True): as bam_markdup takes them; the counts gain "templates_without_barcode".
    barcode_edits (needs a barcode source): as bam_markdup takes it; the counts gain BARCODE_GROUP_COUNTS' names.
    optical_distance: the record's field, which the library refuses here -- a stand-alone file has no optical step (bam_markdup counts optical duplicates)."""
    L = _sorted_file_api(load_library())
    if apply_recal_report is not None and apply_recal is None:
        raise ValueError("bam_sorted_file: apply_recal_report needs apply_recal (it says what the applied table changed)")
    if apply_recal is not None:
        recal = dict(recal, apply=apply_recal) if recal is not None else dict(apply=apply_recal, count=False)
    q = sorted_request("bam_sorted_file", L, markdup=markdup, read_groups=read_groups, optical_distance=optical_distance, barcode_tag=barcode_tag, barcode_name=barcode_name, barcode_edits=barcode_edits, coverage=coverage,
                       stats=stats, index_format=index_format, csi_min_shift=csi_min_shift, level=level, window=window, recal=recal)
    records = bytes(records)
    names = (C.c_char_p * max(len(contigs), 1))(*[c[0].encode() for c in contigs])
    lens = np.ascontiguousarray([c[1] for c in contigs] or [0], dtype=np.int64)
    if q.opt.index_format == INDEX_BAI and ((lens < 0) | (lens >= 1 << 29)).any():
        raise ValueError("bam_sorted_file: a BAI index holds contigs below 2^29 bases (CSI is not written)")
    if ((lens < 0) | (lens >= 1 << 31)).any():
        raise ValueError("bam_sorted_file: BAM and its CSI index hold contigs of at most 2^31 - 1 bases")
    lens = lens.astype(np.int32)
    bam, bai, nb, ni = C.c_void_p(), C.c_void_p(), C.c_uint64(), C.c_uint64()
    rc = (L.bmh_bam_sorted_file_host if host else L.bmh_bam_sorted_file_device)(header_text.encode(), len(contigs), names, lens.ctypes.data, records, len(records), C.byref(q.opt), *([] if host else [_current_stream()]),
              C.byref(bam), C.byref(nb), C.byref(bai), C.byref(ni), C.byref(q.res))
    if rc != 0:
        raise (ValueError if rc == -2 else RuntimeError)("bmh_bam_sorted_file: " + _err(L))
    try:
        got = q.results(L)
        if apply_recal_report is not None:
            from .recal import write_recal_apply_report
            write_recal_apply_report(got["recal"]["apply"], apply_recal_report)
        return (C.string_at(bam.value, nb.value), C.string_at(bai.value, ni.value)) + tuple(got[k] for k in ("markdup", "coverage", "stats", "recal") if k in got)
    finally:
        L.bmh_free.argtypes = [C.c_void_p]
        L.bmh_free(bam); L.bmh_free(bai)


class CoverageOpt(C.Structure):
    """bmh_coverage_opt_t"""
    _fields_ = [("min_mapq", C.c_int32), ("deletions", C.c_int32), ("bin", C.c_uint32), ("tile", C.c_uint32)]


class Coverage(C.Structure):
    """bmh_coverage_t"""
    _fields_ = [("n_contigs", C.c_int32), ("n_bins", C.c_uint64), ("n_reads", _u64p), ("cov_bases", _u64p), ("sum_depth", _u64p), ("max_depth", _u64p), ("sum_mapq", _u64p),
                ("hist", _u64p), ("bin_sum", _u64p)]


COVERAGE_CONTIG_ARRAYS = ("n_reads", "cov_bases", "sum_depth", "max_depth", "sum_mapq")
COVERAGE_HIST = 1001


def coverage_opt(min_mapq=0, deletions=False, bin=0, tile=0, what="bam_coverage") -> CoverageOpt:
    """the coverage keywords, checked -> bmh_coverage_opt_t; ValueError names the keyword"""
    for nm, v, lo, hi in (("min_mapq", min_mapq, 0, 255), ("bin", bin, 0, 0xffffffff), ("tile", tile, 0, 4096)):
        if not isinstance(v, (int, np.integer)) or isinstance(v, bool) or not lo <= v <= hi:
            raise ValueError(f"{what}: {nm} {v!r}: an integer in {lo} .. {hi}")
    return CoverageOpt(int(min_mapq), 1 if deletions else 0, int(bin), int(tile))


def coverage_dict(L, cov: Coverage) -> dict:
    """bmh_coverage_t -> {name: numpy array of uint64}; the record's arrays are released"""
    try:
        out = {nm: np.ctypeslib.as_array(getattr(cov, nm), shape=(max(cov.n_contigs, 1),))[:cov.n_contigs].copy() for nm in COVERAGE_CONTIG_ARRAYS}
        out["hist"] = np.ctypeslib.as_array(cov.hist, shape=(COVERAGE_HIST,)).copy()
        out["bin_sum"] = np.ctypeslib.as_array(cov.bin_sum, shape=(max(int(cov.n_bins), 1),))[:int(cov.n_bins)].copy()
        return out
    finally:
        L.bmh_free.argtypes = [C.c_void_p]
        for nm in COVERAGE_CONTIG_ARRAYS + ("hist", "bin_sum"):
            L.bmh_free(C.cast(getattr(cov, nm), C.c_void_p))


def bam_coverage(records: bytes, contigs, host: bool = False, min_mapq: int = 0, deletions: bool = False, bin: int = 0, tile: int = 0) -> dict:
    """bmh_bam_coverage_device (host=True: _host, no device needed): a stream of BAM records in coordinate order and the contigs ((name, length) pairs, or
    lengths) -> the coverage depth as a dict of uint64 arrays: per contig n_reads, cov_bases, sum_depth, max_depth, sum_mapq; hist [1001]
    (positions of all contigs at depth d, the last bin 1000 and more, depth 0 included); bin_sum (with bin=B: the depth summed over every B positions, contig
    after contig).  `samtools depth`'s default filters (flags 0x4 0x100 0x200 0x400 out, mapq >= min_mapq); deletions=True: D covers (-J).  tile: the positions
    swept at once (0: 4096) -- no result depends on it.  A stream out of order, a counted record that begins outside its contig or holds the long-CIGAR
    placeholder, and 2^28 bins or more raise ValueError."""
    L = load_library()
    records = bytes(records)
    o = coverage_opt(min_mapq, deletions, bin, tile)
    lens = np.ascontiguousarray([c[1] if isinstance(c, (tuple, list)) else c for c in contigs] or [0], dtype=np.int64)
    if ((lens < 0) | (lens >= 1 << 31)).any():
        raise ValueError("bam_coverage: BAM holds contigs of at most 2^31 - 1 bases")
    lens = lens.astype(np.int32)
    cov = Coverage()
    head = [C.c_char_p, C.c_uint64, C.c_int, C.c_void_p, C.POINTER(CoverageOpt)]
    if host:
        L.bmh_bam_coverage_host.argtypes = head + [C.POINTER(Coverage)]
        rc = L.bmh_bam_coverage_host(records, len(records), len(contigs), lens.ctypes.data, C.byref(o), C.byref(cov))
    else:
        import torch
        L.bmh_bam_coverage_device.argtypes = head + [C.c_void_p, C.POINTER(Coverage)]
        rc = L.bmh_bam_coverage_device(records, len(records), len(contigs), lens.ctypes.data, C.byref(o), torch.cuda.current_stream().cuda_stream, C.byref(cov))
    if rc != 0:
        raise (ValueError if rc == -2 else RuntimeError)("bmh_bam_coverage: " + _err(L))
    return coverage_dict(L, cov)


class BamStatsOpt(C.Structure):
    """bmh_bam_stats_opt_t"""
    _fields_ = [("insert_cap", C.c_uint32)]


class BamStats(C.Structure):
    """bmh_bam_stats_t"""
    _fields_ = [("n_contigs", C.c_int32), ("insert_cap", C.c_uint32), ("flag", _u64p), ("summary", _u64p), ("mapq", _u64p), ("contig_mapped", _u64p), ("contig_unmapped", _u64p),
                ("insert_hist", _u64p), ("unplaced", C.c_uint64), ("insert_min", C.c_uint64 * 3), ("insert_max", C.c_uint64 * 3)]


BAM_STATS_FLAGS = ("total", "primary", "secondary", "supplementary", "duplicates", "primary_duplicates", "mapped", "primary_mapped", "paired", "read1", "read2", "properly_paired",
                   "both_mapped", "singletons", "mate_on_different_contig", "mate_on_different_contig_mapq5")
BAM_STATS_SUMMARY = ("reads", "bases", "reads_mapped", "bases_mapped", "reads_mq0", "max_read_length", "bases_aligned", "bases_soft_clipped", "ins_events", "ins_bases", "del_events",
                     "del_bases", "reads_with_nm", "edit_distance")
BAM_STATS_ORIENTATIONS = ("FR", "RF", "TANDEM")
INSERT_CAP_DEFAULT = 65536


def stats_opt(insert_cap=INSERT_CAP_DEFAULT, what="bam_stats") -> BamStatsOpt:
    """the statistics' keyword, checked -> bmh_bam_stats_opt_t; ValueError names the keyword"""
    if insert_cap is None:
        insert_cap = INSERT_CAP_DEFAULT
    if not isinstance(insert_cap, (int, np.integer)) or isinstance(insert_cap, bool) or not 2 <= insert_cap <= 65536:
        raise ValueError(f"{what}: insert_cap {insert_cap!r}: an integer in 2 .. 65536")
    return BamStatsOpt(int(insert_cap))


def stats_dict(L, st: BamStats) -> dict:
    """bmh_bam_stats_t -> {name: numpy array of uint64}; the record's arrays are released"""
    L.bmh_bam_stats_free.argtypes, L.bmh_bam_stats_free.restype = [C.POINTER(BamStats)], None
    try:
        n, cap = int(st.n_contigs), int(st.insert_cap)
        out = dict(flag=np.ctypeslib.as_array(st.flag, shape=(2, 16)).copy(), summary=np.ctypeslib.as_array(st.summary, shape=(14,)).copy(),
                   mapq=np.ctypeslib.as_array(st.mapq, shape=(256,)).copy(), insert_hist=np.ctypeslib.as_array(st.insert_hist, shape=(3, cap + 1)).copy())
        for nm in ("contig_mapped", "contig_unmapped"):
            out[nm] = np.ctypeslib.as_array(getattr(st, nm), shape=(max(n, 1),))[:n].copy()
        out["unplaced"] = np.array([st.unplaced], dtype=np.uint64)
        out["insert_min"] = np.array(list(st.insert_min), dtype=np.uint64); out["insert_max"] = np.array(list(st.insert_max), dtype=np.uint64)
        return out
    finally:
        L.bmh_bam_stats_free(C.byref(st))


def bam_stats(records: bytes, n_contigs: int, insert_cap: int = INSERT_CAP_DEFAULT, host: bool = False) -> dict:
    """bmh_bam_stats_device (host=True: _host, no device needed): a stream of BAM records in any order among n_contigs contigs -> the statistics of DESIGN.md 4.15
    as a dict of uint64 arrays, device and host integer for integer the same: flag [2][16] (`samtools flagstat`'s counts by BAM_STATS_FLAGS' names; row 1: the
    records with 0x200), contig_mapped / contig_unmapped [n_contigs] and unplaced [1] (`samtools idxstats`), summary [14] (BAM_STATS_SUMMARY's names, over primary
    records), mapq [256] (mapped primary records), insert_hist [3][insert_cap + 1] (FR, RF, TANDEM; sizes from insert_cap up in the last bin), insert_min /
    insert_max [3] (exact; 0 without a pair).  flagstat_text, idxstats_text, stats_text and insert_size_metrics (bwamem_hip.aligner) make the texts.  A refID outside
    the contigs, and of mapped primary records damaged tags, an NM that is no count and the long-CIGAR placeholder raise ValueError naming the record."""
    L = load_library()
    records = bytes(records)
    o = stats_opt(insert_cap)
    if not isinstance(n_contigs, (int, np.integer)) or isinstance(n_contigs, bool) or not 0 <= n_contigs < 1 << 31:
        raise ValueError(f"bam_stats: n_contigs {n_contigs!r}: a number of contigs")
    st = BamStats()
    head = [C.c_char_p, C.c_uint64, C.c_int, C.POINTER(BamStatsOpt)]
    if host:
        L.bmh_bam_stats_host.argtypes = head + [C.POINTER(BamStats)]
        rc = L.bmh_bam_stats_host(records, len(records), int(n_contigs), C.byref(o), C.byref(st))
    else:
        import torch
        L.bmh_bam_stats_device.argtypes = head + [C.c_void_p, C.POINTER(BamStats)]
        rc = L.bmh_bam_stats_device(records, len(records), int(n_contigs), C.byref(o), torch.cuda.current_stream().cuda_stream, C.byref(st))
    if rc != 0:
        raise (ValueError if rc == -2 else RuntimeError)("bmh_bam_stats: " + _err(L))
    return stats_dict(L, st)


class Recal(C.Structure):
    """bmh_recal_t (the members from apply_summary on belong to the apply step, DESIGN.md 4.17: the library touches them only where RecalOpt's apply is set)"""
    _fields_ = [("n_groups", C.c_int32), ("min_qual", C.c_int32), ("max_cycle", C.c_int32), ("n_qual", C.c_int32), ("summary", C.c_uint64 * 16),
                ("cycle_m", _u64p), ("cycle_id", _u64p), ("context_m", _u64p), ("context_id", _u64p),
                ("apply_summary", C.c_uint64 * 16), ("qual_hist", _u64p), ("apply_ms", C.c_double), ("apply_windows", C.c_uint64)]


class RecalApplyOpt(C.Structure):
    """bmh_recal_apply_opt_t"""
    _fields_ = [("table", C.POINTER(Recal)), ("rg_ids", C.POINTER(C.c_char_p))]


class RecalOpt(C.Structure):
    """bmh_recal_opt_t"""
    _fields_ = [("min_qual", C.c_int32), ("max_cycle", C.c_int32), ("pac", C.c_void_p), ("l_pac", C.c_uint64), ("contig_offset", C.c_void_p), ("mask", C.c_void_p),
                ("mask_words", C.c_uint64), ("n_groups", C.c_int32), ("rg_ids", C.POINTER(C.c_char_p)), ("apply", C.POINTER(RecalApplyOpt)), ("no_count", C.c_int32)]


RECAL_SUMMARY = ("records_seen", "records_counted", "left_out_no_contig", "left_out_flags", "left_out_mapq", "left_out_no_qualities", "left_out_no_operations", "bases_kept",
                 "skipped_not_acgt", "skipped_low_quality", "skipped_masked", "skipped_masked_anchor", "cycles_capped", "masked_positions")
RECAL_MIN_QUAL, RECAL_MAX_CYCLE, RECAL_INDEL_QUAL, RECAL_MAX_GROUPS = 6, 500, 45, 255
RECAL_APPLY_SUMMARY = ("records_seen", "records_rewritten", "records_without_qualities", "bases_seen", "bases_below_min_qual", "bases_changed", "bases_unchanged", "cycles_capped",
                       "bases_without_context")
RECAL_WIDE = 1      # summary[15] of a bmh_recal_t that holds the apply step's members


def recal_apply_opt(table, what="bam_apply_recal"):
    """a table to apply (read_recal_table's / bam_recal's dict, or a path to the text) -> (bmh_recal_apply_opt_t, what it points to, to be kept alive as long as it).
    ValueError names what the dict lacks; the library checks the rows"""
    if isinstance(table, (str, bytes, os.PathLike)):
        from .recal import read_recal_table
        table = read_recal_table(os.fspath(table))
    if not isinstance(table, dict) or any(k not in table for k in ("cycle_m", "context_m", "min_qual", "max_cycle")):
        raise ValueError(f"{what}: apply_recal takes a path or read_recal_table's dict (cycle_m, context_m, min_qual, max_cycle, read_groups)")
    cy, cx = np.ascontiguousarray(table["cycle_m"], dtype=np.uint64), np.ascontiguousarray(table["context_m"], dtype=np.uint64)
    c = int(table["max_cycle"])
    if cy.ndim != 4 or cx.ndim != 4 or cy.shape[1:] != (94, 2 * c, 2) or cx.shape != (cy.shape[0], 94, 17, 2):
        raise ValueError(f"{what}: apply_recal: cycle_m {cy.shape} and context_m {cx.shape} are not [groups][94][2 max_cycle][2] and [groups][94][17][2] at max_cycle {c}")
    ids = [str(g) for g in (table.get("read_groups") or ["*"])]
    if len(ids) != cy.shape[0]:
        raise ValueError(f"{what}: apply_recal: {len(ids)} read groups for a table of {cy.shape[0]}")
    rt = Recal(cy.shape[0], int(table["min_qual"]), c, 94)
    rt.cycle_m, rt.context_m = cy.ctypes.data_as(_u64p), cx.ctypes.data_as(_u64p)
    arr = (C.c_char_p * len(ids))(*[g.encode() for g in ids])
    a = RecalApplyOpt(C.pointer(rt), arr)
    return a, [cy, cx, rt, arr]


def recal_opt(what="bam_recal", pac=None, l_pac=0, contig_offset=None, mask=None, read_groups=None, min_qual=None, max_cycle=None, known_sites=None, apply=None, count=True):
    """the recalibration table's keywords, checked -> (bmh_recal_opt_t, what it points to, to be kept alive as long as it); ValueError names the keyword.
    pac: the .pac body (bytes or a uint8 array; None where the caller holds the reference: an aligner's run), l_pac its bases, contig_offset every contig's
    first base in it (None: back to back), mask a uint64 array of (l_pac + 63) // 64 words (known_sites_mask), read_groups the IDs in table order (None: the
    one group `*`).  known_sites is not read here: the names go into the text.  apply: a table to apply to the qualities as they are written (recal_apply_opt's
    argument); count=False (needs apply): apply only -- no table is counted and nothing but apply is read"""
    min_qual = RECAL_MIN_QUAL if min_qual is None else min_qual
    max_cycle = RECAL_MAX_CYCLE if max_cycle is None else max_cycle
    if not isinstance(min_qual, (int, np.integer)) or isinstance(min_qual, bool) or not 0 <= min_qual <= 93:
        raise ValueError(f"{what}: recal_min_qual {min_qual!r}: an integer in 0 .. 93")
    if not isinstance(max_cycle, (int, np.integer)) or isinstance(max_cycle, bool) or not 1 <= max_cycle <= 65535:
        raise ValueError(f"{what}: recal_max_cycle {max_cycle!r}: an integer in 1 .. 65535")
    keep = []
    o = RecalOpt(int(min_qual), int(max_cycle))
    if pac is not None:
        a = np.frombuffer(bytes(pac), dtype=np.uint8) if isinstance(pac, (bytes, bytearray, memoryview)) else np.ascontiguousarray(pac, dtype=np.uint8)
        if a.size < (int(l_pac) + 3) // 4:
            raise ValueError(f"{what}: pac holds {a.size} bytes, {int(l_pac)} bases take {(int(l_pac) + 3) // 4}")
        a = np.concatenate([a, np.zeros(8, np.uint8)])
        keep.append(a); o.pac = a.ctypes.data
    o.l_pac = int(l_pac)
    if contig_offset is not None:
        a = np.ascontiguousarray(contig_offset, dtype=np.uint64)
        keep.append(a); o.contig_offset = a.ctypes.data
    if mask is not None:
        a = np.ascontiguousarray(mask, dtype=np.uint64)
        keep.append(a); o.mask = a.ctypes.data; o.mask_words = a.size
    if read_groups is not None:
        ids = [str(g) for g in read_groups]
        if len(ids) > RECAL_MAX_GROUPS:
            raise ValueError(f"{what}: {len(ids)} read groups: the recalibration table holds at most {RECAL_MAX_GROUPS}")
        if ids:
            arr = (C.c_char_p * len(ids))(*[g.encode() for g in ids])
            keep.append(arr); o.n_groups = len(ids); o.rg_ids = arr
    if not count and apply is None:
        raise ValueError(f"{what}: count=False needs apply (a run that neither counts nor applies a table has no recalibration step)")
    if apply is not None:
        a, held = recal_apply_opt(apply, what)
        keep += [a] + held; o.apply = C.pointer(a); o.no_count = 0 if count else 1
    return o, keep


def recal_dict(L, rt: Recal, read_groups=None, known_sites=None) -> dict:
    """bmh_recal_t -> {name: numpy array of uint64} and the run's parameters; the record's arrays are released"""
    L.bmh_recal_free.argtypes, L.bmh_recal_free.restype = [C.POINTER(Recal)], None
    try:
        g, c, nq = int(rt.n_groups), int(rt.max_cycle), int(rt.n_qual)
        out = {}
        if rt.cycle_m:                                             # (an apply-only run counts no table)
            summary = np.array(list(rt.summary), dtype=np.uint64); summary[15] = 0
            out = dict(summary=summary, cycle_m=np.ctypeslib.as_array(rt.cycle_m, shape=(g, nq, 2 * c, 2)).copy(),
                       cycle_id=np.ctypeslib.as_array(rt.cycle_id, shape=(g, 2 * c, 3)).copy(), context_m=np.ctypeslib.as_array(rt.context_m, shape=(g, nq, 17, 2)).copy(),
                       context_id=np.ctypeslib.as_array(rt.context_id, shape=(g, 65, 3)).copy(), min_qual=int(rt.min_qual), max_cycle=c,
                       read_groups=[str(x) for x in read_groups] if read_groups else ["*"], known_sites=[str(p) for p in (known_sites or [])])
        if rt.summary[15] == RECAL_WIDE:                           # the apply step's counts
            s = np.array(list(rt.apply_summary), dtype=np.uint64)
            out["apply"] = dict(summary=s, qual_hist=np.ctypeslib.as_array(rt.qual_hist, shape=(2, 94)).copy(), ms=(float(rt.apply_ms), int(rt.apply_windows)),
                                **dict(zip(RECAL_APPLY_SUMMARY, (int(v) for v in s))))
        return out
    finally:
        L.bmh_recal_free(C.byref(rt))


def bam_recal(records: bytes, contigs, pac, l_pac: int, mask=None, read_groups=None, min_qual: int = RECAL_MIN_QUAL, max_cycle: int = RECAL_MAX_CYCLE, host: bool = False,
              contig_offset=None) -> dict:
    """bmh_bam_recal_device (host=True: _host, no device needed): a stream of BAM records in any order over `contigs` ((name, length) pairs, or lengths) and the
    reference's .pac body -> the covariate table of DESIGN.md 4.16 as a dict of uint64 arrays, device and host integer for integer the same: summary [16]
    (RECAL_SUMMARY's names), cycle_m [groups][94][2 max_cycle][2] (event M: observations, errors; slot max_cycle + c - 1 for cycle c > 0, max_cycle + c for
    c < 0), cycle_id [groups][2 max_cycle][3] (events I and D at quality 45: their observations, insertion errors, deletion errors), context_m
    [groups][94][17][2] (context 4 a + b, 16: none), context_id [groups][65][3] (16 a + 4 b + c, 64: none); and min_qual, max_cycle, read_groups, known_sites.
    recal_table_text (bwamem_hip.recal) makes the text.  A refused record raises ValueError naming its index."""
    L = load_library()
    records = bytes(records)
    lens = np.ascontiguousarray([c[1] if isinstance(c, (tuple, list)) else c for c in contigs] or [0], dtype=np.int32)
    o, keep = recal_opt("bam_recal", pac, l_pac, contig_offset, mask, read_groups, min_qual, max_cycle)
    rt = Recal()
    head = [C.c_char_p, C.c_uint64, C.c_int, C.c_void_p, C.POINTER(RecalOpt)]
    if host:
        L.bmh_bam_recal_host.argtypes = head + [C.POINTER(Recal)]
        rc = L.bmh_bam_recal_host(records, len(records), len(contigs), lens.ctypes.data, C.byref(o), C.byref(rt))
    else:
        L.bmh_bam_recal_device.argtypes = head + [C.c_void_p, C.POINTER(Recal)]
        rc = L.bmh_bam_recal_device(records, len(records), len(contigs), lens.ctypes.data, C.byref(o), _current_stream(), C.byref(rt))
    if rc != 0:
        raise (ValueError if rc == -2 else RuntimeError)("bmh_bam_recal: " + _err(L))
    return recal_dict(L, rt, read_groups)


def bam_apply_recal(records: bytes, table, host: bool = False) -> tuple:
    """bmh_bam_requal_device (host=True: _host, no device needed): a stream of BAM records in any order and a recalibration table (read_recal_table's dict or a
    path) -> (the same stream with the base qualities rewritten as DESIGN.md 4.17 says, the counts: "summary" [16] with RECAL_APPLY_SUMMARY's names beside it,
    "qual_hist" [2][94] the qualities before and after).  Device and host give the same bytes.  A refused record raises ValueError naming its index, a refused
    table one naming the row"""
    L = load_library()
    records = bytes(records)
    a, keep = recal_apply_opt(table)
    rt, out = Recal(), C.c_void_p()
    head = [C.c_char_p, C.c_uint64, C.POINTER(RecalApplyOpt)]
    if host:
        L.bmh_bam_requal_host.argtypes = head + [C.POINTER(C.c_void_p), C.POINTER(Recal)]
        rc = L.bmh_bam_requal_host(records, len(records), C.byref(a), C.byref(out), C.byref(rt))
    else:
        L.bmh_bam_requal_device.argtypes = head + [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(Recal)]
        rc = L.bmh_bam_requal_device(records, len(records), C.byref(a), _current_stream(), C.byref(out), C.byref(rt))
    if rc != 0:
        raise (ValueError if rc == -2 else RuntimeError)("bmh_bam_requal: " + _err(L))
    try:
        return C.string_at(out.value, len(records)), recal_dict(L, rt)["apply"]
    finally:
        L.bmh_free.argtypes = [C.c_void_p]
        L.bmh_free(out)


def recal_apply_tables(table) -> np.ndarray:
    """bmh_recal_apply_tables: the int16 deltas both forms of the apply step read, [groups][94][1 + 2 max_cycle + 16] -- b, the cycle deltas, the context deltas,
    in 1/256 of a quality.  A refused table raises ValueError naming the row"""
    L = load_library()
    a, keep = recal_apply_opt(table, "recal_apply_tables")
    out, n = C.c_void_p(), C.c_uint64()
    L.bmh_recal_apply_tables.argtypes = [C.POINTER(RecalApplyOpt), C.POINTER(C.c_void_p), _u64p]
    rc = L.bmh_recal_apply_tables(C.byref(a), C.byref(out), C.byref(n))
    if rc != 0:
        raise (ValueError if rc == -2 else RuntimeError)("bmh_recal_apply_tables: " + _err(L))
    try:
        g = int(a.table.contents.n_groups)
        return np.frombuffer(C.string_at(out.value, 2 * n.value), dtype=np.int16).reshape(g, 94, -1).copy()
    finally:
        L.bmh_free.argtypes = [C.c_void_p]
        L.bmh_free(out)


def requal_kernel_limits() -> dict:
    """bmh_requal_kernel_limits: the constants of the apply step's device form, for the tests that sit on them"""
    L = load_library()
    out = (C.c_uint32 * 3)()
    L.bmh_requal_kernel_limits.argtypes, L.bmh_requal_kernel_limits.restype = [C.POINTER(C.c_uint32)], None
    L.bmh_requal_kernel_limits(out)
    return dict(zip(("lanes", "block_records", "lds_bases"), (int(v) for v in out)))


def known_sites_mask(paths, contigs, l_pac=None, contig_offset=None, holes=None) -> np.ndarray:
    """bmh_known_sites_mask and bmh_recal_mask_holes: the known-sites files `paths` (VCF or BED text, plain or gzip) over `contigs` ((name, length) pairs) and the
    reference's holes ((offset, length) pairs in pac: the .amb's) -> the mask, a uint64 array of (l_pac + 63) // 64 words (l_pac None: the contigs' total).  A line
    that cannot be taken raises ValueError naming file and line"""
    L = load_library()
    paths = [paths] if isinstance(paths, (str, bytes, os.PathLike)) else list(paths or [])
    lens = np.ascontiguousarray([c[1] for c in contigs] or [0], dtype=np.int32)
    total = int(sum(int(c[1]) for c in contigs)) if l_pac is None else int(l_pac)
    mask = np.zeros((total + 63) // 64, dtype=np.uint64)
    names = (C.c_char_p * max(len(contigs), 1))(*[c[0].encode() for c in contigs])
    off = np.ascontiguousarray(contig_offset, dtype=np.uint64) if contig_offset is not None else None
    ps = (C.c_char_p * max(len(paths), 1))(*[os.fsencode(p) for p in paths])
    L.bmh_known_sites_mask.argtypes = [C.POINTER(C.c_char_p), C.c_int, C.c_int, C.POINTER(C.c_char_p), C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64]
    rc = L.bmh_known_sites_mask(ps, len(paths), len(contigs), names, lens.ctypes.data, off.ctypes.data if off is not None else None, mask.ctypes.data, mask.size)
    if rc != 0:
        raise (ValueError if rc == -2 else RuntimeError)("bmh_known_sites_mask: " + _err(L))
    if holes:
        ho = np.ascontiguousarray([h[0] for h in holes], dtype=np.uint64); hl = np.ascontiguousarray([h[1] for h in holes], dtype=np.uint64)
        L.bmh_recal_mask_holes.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_uint64]
        if L.bmh_recal_mask_holes(ho.ctypes.data, hl.ctypes.data, len(holes), mask.ctypes.data, mask.size) != 0:
            raise ValueError("bmh_recal_mask_holes: " + _err(L))
    return mask


def recal_kernel_limits() -> dict:
    """bmh_recal_kernel_limits: the capacities of the device form, for the tests that sit on them"""
    L = load_library()
    out = (C.c_uint32 * 5)()
    L.bmh_recal_kernel_limits.argtypes, L.bmh_recal_kernel_limits.restype = [C.POINTER(C.c_uint32)], None
    L.bmh_recal_kernel_limits(out)
    return dict(zip(("slots", "lanes", "lds_cycles", "block_records", "lds_bases"), (int(v) for v in out)))


def reads_last_bam_counts() -> dict:
    """bmh_reads_last_bam_counts: what the process's last load_reads_files / run_files / bam_reads call left out of its BAM input -- records skipped (flag 0x100
    or 0x800), f and B tags left out of the comments"""
    L = load_library()
    L.bmh_reads_last_bam_counts.argtypes = [C.POINTER(C.c_uint64)]
    out = (C.c_uint64 * 2)()
    L.bmh_reads_last_bam_counts(out)
    return dict(records_skipped=int(out[0]), tags_left_out=int(out[1]))


class SortedOpt(C.Structure):
    """bmh_sorted_opt_t"""
    _fields_ = [("level", C.c_int32), ("window", C.c_uint32), ("index_format", C.c_int32), ("min_shift", C.c_int32), ("sort_mem", C.c_uint64), ("tmp_dir", C.c_char_p),
                ("markdup", C.POINTER(MarkdupOpt)), ("coverage", C.POINTER(CoverageOpt)), ("stats", C.POINTER(BamStatsOpt)), ("recal", C.POINTER(RecalOpt))]


class SortedResults(C.Structure):
    """bmh_sorted_results_t"""
    _fields_ = [("markdup", C.POINTER(MarkdupCounts)), ("coverage", C.POINTER(Coverage)), ("stats", C.POINTER(BamStats)), ("parts", C.c_uint32), ("n_libraries", C.c_int32),
                ("markdup_ms", C.c_double * 2), ("optical_ms", C.c_double), ("coverage_ms", C.c_double), ("stats_ms", C.c_double),
                ("markdup_d2h_bytes", C.c_uint64), ("coverage_windows", C.c_uint64), ("stats_windows", C.c_uint64),
                ("recal", C.POINTER(Recal)), ("recal_ms", C.c_double), ("recal_windows", C.c_uint64)]


SortedFileOpt = SortedOpt      # (the name the record had while it served bmh_bam_sorted_file_* alone: code that imports it gets the one record)


SORTED_PARTS = dict(markdup=1, optical=2, barcode=4, grouped=8, coverage=16, stats=32, recal=64)      # BMH_SORTED_*


def _current_stream() -> int:
    import torch
    return torch.cuda.current_stream().cuda_stream


class SortedRequest:
    """what one sorted output is made under and where its results go, as the library takes them: opt (bmh_sorted_opt_t), res (bmh_sorted_results_t) and every
    record the two point to, kept alive here"""

    def results(self, L, lib_names=None) -> dict:
        """after a call that succeeded: {"markdup": bam_markdup's counts, "coverage": bam_coverage's arrays, "stats": bam_stats' arrays}, each where it was asked
        for (the records' arrays are released)"""
        out = {}
        if self.opt.markdup:
            out["markdup"] = _markdup_dict(self.mo, self.mc, self.lib_names if lib_names is None else lib_names, self.read_groups or lib_names is not None)
        if self.opt.coverage:
            out["coverage"] = coverage_dict(L, self.cov)
        if self.opt.stats:
            out["stats"] = stats_dict(L, self.st)
        if self.opt.recal:
            out["recal"] = recal_dict(L, self.rt, self.recal_kw.get("read_groups"), self.recal_kw.get("known_sites"))
        return out


def sorted_request(what: str, L, markdup: bool = False, read_groups=None, optical_distance=None, barcode_tag=None, barcode_name=None, barcode_edits=None, coverage=None, stats=None,
                   index_format: str = "bai", csi_min_shift: int = 14, level: int = 1, window: int = 0, sort_mem=None, sort_tmp=None, libraries: int = 0, recal=None) -> SortedRequest:
    """the keywords of every sorted output (bam_sorted_file, bam_post, NativeAligner.set_sorted), checked -> a SortedRequest.  ValueError names the keyword: the
    barcode keywords, optical_distance and read_groups need markdup=True; barcode_edits needs a barcode source; index_format "bai" or "csi" with csi_min_shift
    10 .. 24; level 0 or 1; sort_mem a number of bytes.  libraries: room for that many libraries' rows in the counts record where read_groups are not given (the
    callers whose libraries come from elsewhere)"""
    bc_mode, bc_tag = barcode_source(barcode_tag, barcode_name, what)
    if barcode_edits is not None and not markdup:
        raise ValueError(f"{what}: barcode_edits needs markdup=True (barcodes are grouped where duplicates are marked)")
    edits = barcode_edits_value(barcode_edits, bc_mode, what)
    if bc_mode != BARCODE_OFF and not markdup:
        raise ValueError(f"{what}: barcode_tag / barcode_name need markdup=True (barcodes are compared where duplicates are marked)")
    if optical_distance is not None and not markdup:
        raise ValueError(f"{what}: optical_distance needs markdup=True (optical duplicates are counted where duplicates are marked)")
    if read_groups is not None and not markdup:
        raise ValueError(f"{what}: read_groups needs markdup=True (they decide which templates may be duplicates of each other)")
    distance = -1 if optical_distance is None else optical_distance_value(optical_distance, what)
    ix_code, ix_shift = index_format_code(index_format, csi_min_shift, what)
    if level not in (0, 1):
        raise ValueError(f"{what}: level {level}: 0 or 1")
    if sort_mem is not None and (not isinstance(sort_mem, (int, np.integer)) or isinstance(sort_mem, bool) or sort_mem < 1):
        raise ValueError(f"{what}: sort_mem {sort_mem!r}: a number of bytes, 1 and more")
    q = SortedRequest()
    q.read_groups = read_groups is not None
    q.mo, q.mc, q.lib_names, q.keep = _markdup_records(_markdup_api(L), read_groups, distance, 0, bc_mode, bc_tag, edits, 0)
    if libraries and read_groups is None:
        arrays = [(C.c_uint64 * (k * libraries))() for k in (8, 3, 3)]
        q.mc.lib_counts, q.mc.lib_optical, q.mc.lib_grouped = (C.cast(a, _u64p) for a in arrays)
        q.keep = arrays
    q.co = coverage_opt(what=what, **coverage) if coverage is not None else None
    q.so = stats_opt(what=what, **stats) if stats is not None else None
    q.cov, q.st = Coverage(), BamStats()
    q.opt = SortedOpt(int(level), int(window), ix_code, ix_shift, int(sort_mem or 0), os.fsencode(sort_tmp) if sort_tmp is not None else None,
                      C.pointer(q.mo) if markdup else None, C.pointer(q.co) if q.co is not None else None, C.pointer(q.so) if q.so is not None else None)
    q.res = SortedResults(C.pointer(q.mc) if markdup else None, C.pointer(q.cov) if q.co is not None else None, C.pointer(q.st) if q.so is not None else None)
    q.recal_kw, q.rt = {k: v for k, v in (recal or {}).items() if k not in ("apply", "count")}, Recal()
    if recal is not None:                                          # (recal_opt's keywords; the record is the options' and the results' last member)
        q.ro, q.recal_keep = recal_opt(what, **recal)
        q.recal_kw = {k: v for k, v in recal.items() if k not in ("apply", "count")}
        q.opt.recal = C.pointer(q.ro); q.res.recal = C.pointer(q.rt)
    return q


def _sorted_file_api(L):
    """the library with the argument types of bmh_bam_sorted_file_host and _device"""
    head = [C.c_char_p, C.c_int, C.POINTER(C.c_char_p), C.c_void_p, C.c_char_p, C.c_uint64, C.POINTER(SortedOpt)]
    out = [C.POINTER(C.c_void_p), _u64p, C.POINTER(C.c_void_p), _u64p, C.POINTER(SortedResults)]
    L.bmh_bam_sorted_file_host.argtypes, L.bmh_bam_sorted_file_device.argtypes = head + out, head + [C.c_void_p] + out
    L.bmh_sorted_opt_default.argtypes, L.bmh_sorted_opt_default.restype = [C.POINTER(SortedOpt)], None
    return L


class BamPostOpt(C.Structure):
    """bmh_bam_post_opt_t"""
    _fields_ = [("sorted", SortedOpt), ("batch_bytes", C.c_uint64), ("libraries", C.c_int32), ("collate", C.c_int32)]


class BamPostResult(C.Structure):
    """bmh_bam_post_result_t"""
    _fields_ = [("index", C.c_void_p), ("index_bytes", C.c_uint64), ("header_text", C.c_void_p), ("header_bytes", C.c_uint64), ("n_contigs", C.c_int32), ("contig_names", C.c_void_p),
                ("contig_len", C.POINTER(C.c_int32)), ("n_libraries", C.c_int32), ("library_names", C.c_void_p), ("counts", C.c_uint64 * 6)]


BAM_POST_COUNTS = ("records", "templates", "batches", "spilled_runs", "bins_changed", "duplicate_flags_cleared")
_SINK = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_size_t)


def _names_blob(addr, n: int) -> list:
    """n NUL-terminated names back to back at addr"""
    out = []
    for _ in range(n):
        s = C.string_at(addr)
        out.append(s.decode("latin-1")); addr += len(s) + 1
    return out


def bam_post(src: str, write, host: bool = False, level: int = 1, window: int = 0, index_format: str = "bai", csi_min_shift: int = 14, sort_mem=None, sort_tmp=None, batch_bytes=None,
             markdup: bool = False, libraries: bool = False, optical_distance=None, barcode_tag=None, barcode_name=None, barcode_edits=None, coverage=None, collate: bool = False, stats=None, recal=None) -> dict:
    """recal={pac, l_pac, ...} (recal_opt's keywords; read_groups: the header's @RG IDs in order, see bam_read_groups): "recal" holds the file's covariate table.
    stats={insert_cap} (bmh_sorted_opt_t's stats; {} for the default): "stats" holds the file's statistics (bam_stats' dict), from the windows of the merge.
    bmh_bam_post_file_device (host=True: bmh_bam_post_file_host, no device needed; it holds the whole record stream in memory): the BAM or SAM file `src` of any
    aligner (a path; plain, gzip or BGZF; a pipe) -> the coordinate-sorted BAM, handed to write(bytes) piece by piece, and a dict: "index" (the .bai or .csi
    bytes), "header" (the output header's text), "contigs" ((name, length) pairs), "counts" (BAM_POST_COUNTS' names), with markdup=True "markdup" (bam_markdup's
    counts; with libraries=True -- the header's @RG lines are the table of libraries -- "libraries" per library), with coverage={min_mapq, deletions, bin, tile}
    "coverage" (bam_coverage's arrays).  DESIGN.md 4.14 has the definition.  The keywords are bam_markdup's and bam_sorted_file's and are refused as there;
    libraries, optical_distance and the barcode keywords need markdup=True.  A refused input raises ValueError naming the record's index or the line's number.
    collate=True (needs markdup=True; the library refuses it otherwise): templates by name over the whole file (BDP_TPL_FILE), so that a coordinate-sorted file can
    be marked -- a template is every record of the file under one read name, adjacent or not; a name whose records are no proper template is refused.  It keeps 32
    bytes per record in host memory (48 / 56 with optical_distance / barcodes) until the last batch is in."""
    what = "bam_post"
    if libraries and not markdup:
        raise ValueError(f"{what}: libraries needs markdup=True (they decide which templates may be duplicates of each other)")
    if batch_bytes is not None and (not isinstance(batch_bytes, (int, np.integer)) or isinstance(batch_bytes, bool) or batch_bytes < 1):
        raise ValueError(f"{what}: batch_bytes {batch_bytes!r}: a number of bytes, 1 and more")
    if batch_bytes is not None and batch_bytes > 1 << 30:
        raise ValueError(f"{what}: batch_bytes {batch_bytes}: at most 2^30")
    L = load_library()
    q = sorted_request(what, L, markdup=markdup, optical_distance=optical_distance, barcode_tag=barcode_tag, barcode_name=barcode_name, barcode_edits=barcode_edits, coverage=coverage,
                       stats=stats, index_format=index_format, csi_min_shift=csi_min_shift, level=level, window=window, sort_mem=sort_mem, sort_tmp=sort_tmp, libraries=255 if libraries else 0, recal=recal)
    o = BamPostOpt(q.opt, int(batch_bytes or 0), 1 if libraries else 0, 1 if collate else 0)
    failed = []

    def sink(_user, p, n):
        try:
            write(C.string_at(p, n))
            return 0
        except BaseException as e:                                 # (an exception must not cross the C frames: the run ends, then it is raised)
            failed.append(e)
            return 1
    cb, out = _SINK(sink), BamPostResult()
    L.bmh_bam_post_result_free.argtypes, L.bmh_bam_post_result_free.restype = [C.POINTER(BamPostResult)], None
    call = L.bmh_bam_post_file_host if host else L.bmh_bam_post_file_device
    call.argtypes = [C.c_char_p, C.POINTER(BamPostOpt)] + ([] if host else [C.c_void_p]) + [_SINK, C.c_void_p, C.POINTER(BamPostResult), C.POINTER(SortedResults)]
    rc = call(os.fsencode(src), C.byref(o), *([] if host else [_current_stream()]), cb, None, C.byref(out), C.byref(q.res))
    if failed:
        raise failed[0]
    if rc != 0:
        raise (ValueError if rc == -2 else RuntimeError)("bmh_bam_post_file: " + _err(L))
    try:
        names = _names_blob(out.contig_names, out.n_contigs)
        r = dict(index=C.string_at(out.index, out.index_bytes), header=C.string_at(out.header_text, out.header_bytes).decode("latin-1"),
                 contigs=[(nm, int(out.contig_len[k])) for k, nm in enumerate(names)], counts=dict(zip(BAM_POST_COUNTS, (int(v) for v in out.counts))))
        r.update(q.results(L, _names_blob(out.library_names, out.n_libraries) if libraries else None))
        return r
    finally:
        L.bmh_bam_post_result_free(C.byref(out))


class BamTemplates(C.Structure):
    """bmh_bam_templates_t"""
    _fields_ = [("n_records", C.c_uint64), ("n_templates", C.c_uint64), ("tpl", C.c_void_p), ("entries", C.c_void_p), ("locs", C.c_void_p), ("barcodes", C.c_void_p),
                ("counts", C.c_uint64 * 3), ("lib_counts", C.c_void_p), ("n_libraries", C.c_int32)]


ENTRY_DTYPE = np.dtype([("lo", "<u8"), ("hi", "<u8"), ("score", "<u4"), ("kind_n", "<u4")])                   # bdp_entry_t; kind_n: kind (0 none, 1 fragment, 2 pair) | records << 2
TEMPLATE_COUNTS = ("secondary_or_supplementary", "unmapped_records", "templates")


def bam_templates(records: bytes, host: bool = False, read_groups=None, barcode_tag=None, barcode_name=None, hash_bits: int = 128, barcode_edits=None) -> dict:
    """bmh_bam_templates_device (host=True: bmh_bam_templates_host, no device needed): the grouping of bam_post(collate=True) on its own (DESIGN.md 4.14,
    BDP_TPL_FILE).  A stream of whole BAM records in any order -> a dict: "tpl" (every record's template ordinal: templates are the records under one read name,
    numbered by their first records in stream order), "entries" (ENTRY_DTYPE, one per template), "locations" (LOCATION_DTYPE), with a barcode source "barcodes"
    (uint64 words; packed with barcode_edits), "counts" (TEMPLATE_COUNTS' names) and with read_groups "libraries" ({library name: the three counts}).  hash_bits
    (1 .. 128) cuts the 128-bit name keys, so that a test can make two names collide.  A record that marking refuses, a first record without a usable read group
    or barcode, and a name whose records are no proper template raise ValueError with the record's index."""
    L = _markdup_api(load_library())
    records = bytes(records)
    what = "bam_templates"
    bc_mode, bc_tag = barcode_source(barcode_tag, barcode_name, what)
    edits = barcode_edits_value(barcode_edits, bc_mode, what)
    if not isinstance(hash_bits, (int, np.integer)) or isinstance(hash_bits, bool) or not 1 <= hash_bits <= 128:
        raise ValueError(f"{what}: hash_bits {hash_bits!r}: an integer in 1 .. 128")
    o, _res, names, _keep = _markdup_records(L, read_groups, -1, 0, bc_mode, bc_tag, edits, 0)
    out = BamTemplates()
    head = [C.c_char_p, C.c_uint64, C.POINTER(MarkdupOpt), C.c_int32]
    L.bmh_bam_templates_free.argtypes, L.bmh_bam_templates_free.restype = [C.POINTER(BamTemplates)], None
    if host:
        L.bmh_bam_templates_host.argtypes = head + [C.POINTER(BamTemplates)]
        rc = L.bmh_bam_templates_host(records, len(records), C.byref(o), int(hash_bits), C.byref(out))
    else:
        import torch
        L.bmh_bam_templates_device.argtypes = head + [C.c_void_p, C.POINTER(BamTemplates)]
        rc = L.bmh_bam_templates_device(records, len(records), C.byref(o), int(hash_bits), torch.cuda.current_stream().cuda_stream, C.byref(out))
    if rc != 0:
        raise (ValueError if rc == -2 else RuntimeError)("bmh_bam_templates: " + _err(L))
    try:
        n, t = int(out.n_records), int(out.n_templates)

        def arr(addr, count, dtype):
            return np.frombuffer(C.string_at(addr, count * np.dtype(dtype).itemsize) if count else b"", dtype=dtype).copy()
        r = dict(tpl=arr(out.tpl, n, "<u4"), entries=arr(out.entries, t, ENTRY_DTYPE), locations=arr(out.locs, t, LOCATION_DTYPE),
                 counts=dict(zip(TEMPLATE_COUNTS, (int(v) for v in out.counts))))
        if bc_mode != BARCODE_OFF:
            r["barcodes"] = arr(out.barcodes, t, "<u8")
        if read_groups is not None:
            lc = arr(out.lib_counts, 3 * int(out.n_libraries), "<u8")
            r["libraries"] = {nm: dict(zip(TEMPLATE_COUNTS, (int(v) for v in lc[3 * k:3 * k + 3]))) for k, nm in enumerate(names)}
        return r
    finally:
        L.bmh_bam_templates_free(C.byref(out))


def bam_header_read_groups(text, markdup: bool = False) -> tuple:
    """bmh_bam_header_read_groups: the @RG lines of a BAM header's text (bytes or str) -> (the lines verbatim, every line's library index by first appearance).
    The text ends at its first NUL, the last line may lack its newline, CR LF is accepted and other lines are ignored.  Raises ValueError naming the line: no
    @RG line, a line without a non-empty ID of at most 255 bytes or with a field that is not XX:value, a repeated ID, more than 65535 groups, and with
    markdup=True more than 255 libraries."""
    L = load_library()
    text = text.encode() if isinstance(text, str) else bytes(text)
    L.bmh_free.argtypes = [C.c_void_p]
    lines, lib, nb, ng = C.c_void_p(), C.c_void_p(), C.c_uint64(), C.c_int32()
    L.bmh_bam_header_read_groups.argtypes = [C.c_char_p, C.c_uint64, C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_uint64), C.POINTER(C.c_void_p), C.POINTER(C.c_int32)]
    rc = L.bmh_bam_header_read_groups(text, len(text), 1 if markdup else 0, C.byref(lines), C.byref(nb), C.byref(lib), C.byref(ng))
    if rc != 0:
        raise (ValueError if rc == -2 else RuntimeError)(_err(L))
    try:
        return C.string_at(lines.value, nb.value).decode("latin-1").split("\n")[:-1], [int(v) for v in (C.c_int32 * ng.value).from_address(lib.value)]
    finally:
        L.bmh_free(lines); L.bmh_free(lib)


def bam_reads(records: bytes, comments: bool = False, host: bool = False, read_groups=None, collate: bool = False, collate_mem=None) -> dict:
    """bmh_bam_reads_device (host=True: bmh_bam_reads_host, no device needed): uncompressed BAM records, without the header, as load_reads_files gives a file's
    reads -- `samtools fastq`'s rules (include/bwamem_hip.h).  Refused records raise ReadFileError naming the record's index.
    read_groups: a list of read group IDs (bmh_bam_reads_groups_*) -- the result gains "groups", the index of every read's RG:Z value in that list; a kept record
    without the tag, with an RG tag of another type or an ID that is not listed, and a pair of two groups are refused the same way.
    collate=True: the mates of a pair are found by name wherever they lie (BMH_READS_COLLATE, include/bwamem_hip.h); a record still open at the end raises
    ReadFileError whose `partial` holds the complete pairs.  collate_mem: the cap on the open records' bytes (bmh_bam_reads_ex)."""
    L = load_library()
    records = bytes(records)
    rs = ReadSetT()
    L.bmh_reads_free.argtypes = [C.POINTER(ReadSetT)]
    flags = (READS_COMMENTS if comments else 0) | (READS_COLLATE if collate else 0)

    def refused(prefix, other):
        msg = _err(L)
        if not msg.startswith("reads file"):
            return other(prefix + msg)
        e = ReadFileError(msg)
        if rs.ascii:                                   # (an open record at the end of a collated input: the complete pairs before it)
            e.partial = _read_set_dict(L, rs)
        return e
    if read_groups is not None:
        ids = (C.c_char_p * max(len(read_groups), 1))(*[(i if isinstance(i, bytes) else str(i).encode()) for i in read_groups])
        fn = L.bmh_bam_reads_groups_host if host else L.bmh_bam_reads_groups_device
        fn.argtypes = [C.c_char_p, C.c_uint64, C.c_int, C.POINTER(C.c_char_p), C.c_int, C.POINTER(ReadSetT)]
        cap = _collate_cap(collate, collate_mem)
        if cap:
            L.bmh_bam_reads_ex.argtypes = [C.c_char_p, C.c_uint64, C.c_int, C.POINTER(C.c_char_p), C.c_int, C.c_uint64, C.POINTER(ReadSetT)]
            rc = L.bmh_bam_reads_ex(records, len(records), flags | (READS_HOST if host else 0), ids, len(read_groups), cap, C.byref(rs))
        else:
            rc = fn(records, len(records), flags, ids, len(read_groups), C.byref(rs))
        if rc != 0:
            raise refused("bmh_bam_reads: ", ValueError)
        return _read_set_dict(L, rs)
    fn = L.bmh_bam_reads_host if host else L.bmh_bam_reads_device
    fn.argtypes = [C.c_char_p, C.c_uint64, C.c_int, C.POINTER(ReadSetT)]
    cap = _collate_cap(collate, collate_mem)
    if cap:
        L.bmh_bam_reads_ex.argtypes = [C.c_char_p, C.c_uint64, C.c_int, C.POINTER(C.c_char_p), C.c_int, C.c_uint64, C.POINTER(ReadSetT)]
        rc = L.bmh_bam_reads_ex(records, len(records), flags | (READS_HOST if host else 0), None, 0, cap, C.byref(rs))
    else:
        rc = fn(records, len(records), flags, C.byref(rs))
    if rc != 0:
        raise refused("bmh_bam_reads: ", RuntimeError)
    return _read_set_dict(L, rs)


def _read_set_dict(L, rs) -> dict:
    """a filled bmh_read_set_t as numpy arrays over the library's own arrays (no copies; freed with the last of them)"""
    owner = _ReadSetOwner(L, rs)

    def arr(ptr, n, dt):
        n = int(n)
        if n == 0 or not ptr:
            return np.zeros(0, dt)
        buf = (C.c_uint8 * (n * np.dtype(dt).itemsize)).from_address(ptr)
        buf._owner = owner
        return np.frombuffer(buf, dtype=dt)
    return dict(ascii=arr(rs.ascii, rs.n_bases, np.uint8), codes=arr(rs.codes, rs.n_bases, np.uint8), offs=arr(rs.offs, rs.n_reads, np.uint64),
                lens=arr(rs.lens, rs.n_reads, np.uint32), names=arr(rs.names, rs.n_name_bytes, np.uint8), name_offs=arr(rs.name_offs, rs.n_reads, np.uint64),
                quals=arr(rs.quals, rs.n_bases, np.uint8) if rs.quals else None,
                comments=arr(rs.comments, rs.n_comment_bytes, np.uint8) if rs.comments else None,
                comment_offs=arr(rs.comment_offs, rs.n_reads, np.uint64) if rs.comments else None,
                groups=arr(rs.groups, rs.n_reads, np.uint32) if rs.groups else None)


def load_reads_files(path1: str, path2: str | None = None, comments: bool = False, host: bool = False, n_threads: int = 0, collate: bool = False, collate_mem=None,
                     keep_rg: bool = False) -> dict:
    """bmh_reads_load_files: one or two read files of any shape (multi-line records, gzip / BGZF, pipes) as load_reads gives them; path2: the mates (reads 2i
    and 2i+1).  A BGZF file that holds a BAM (unaligned, or grouped by read name) is taken in place of a text file, alone.  host=True: the host walker alone
    (no device).  A refused file raises ReadFileError; when one file ends before the other its `partial` attribute holds the complete pairs before the end.
    collate=True (BMH_READS_COLLATE): a paired BAM in any record order -- mates are found by name; text input is refused; a record still open at the file's end
    is refused with the complete pairs in `partial`.  collate_mem: the cap on the open records' bytes (bmh_reads_load_files_ex).
    keep_rg=True (BMH_READS_KEEP_RG): `path1` is a BAM read under its own read groups -- "groups" is the index of every read's @RG line in the header."""
    L = load_library()
    rs = ReadSetT()
    L.bmh_reads_load_files.argtypes = [C.c_char_p, C.c_char_p, C.c_int, C.c_int, C.POINTER(ReadSetT)]
    L.bmh_reads_free.argtypes = [C.POINTER(ReadSetT)]
    L.bmh_reads_load_files_ex.argtypes = [C.c_char_p, C.c_char_p, C.c_int, C.c_int, C.c_uint64, C.POINTER(ReadSetT)]
    rc = L.bmh_reads_load_files_ex(os.fsencode(path1), os.fsencode(path2) if path2 is not None else None, n_threads,
                                   (READS_COMMENTS if comments else 0) | (READS_HOST if host else 0) | (READS_COLLATE if collate else 0) | (READS_KEEP_RG if keep_rg else 0),
                                   _collate_cap(collate, collate_mem), C.byref(rs))
    msg = _err(L) if rc != 0 else ""
    if rc != 0 and not rs.ascii:
        raise ReadFileError(msg) if msg.startswith(("FASTQ:", "reads file", "reads files")) else RuntimeError("bmh_reads_load_files: " + msg)
    d = _read_set_dict(L, rs)
    if rc != 0:
        e = ReadFileError(msg)
        e.partial = d
        raise e
    return d


class ReadGroupT(C.Structure):
    """bmh_read_group_t"""
    _fields_ = [("id", C.c_char_p), ("library", C.c_int32), ("path1", C.c_char_p), ("path2", C.c_char_p)]


class AlignStats(C.Structure):
    """bmh_align_stats_t"""
    _fields_ = [("n_reads", C.c_uint64), ("n_bytes", C.c_uint64), ("n_batches", C.c_uint32), ("n_lanes", C.c_int)] + \
               [(n, C.c_double) for n in ("seconds", "format_seconds", "h2d_seconds", "seed_seconds", "chain_extend_seconds", "tail_seconds", "select_seconds", "cigar_seconds", "gate_wait_seconds", "h2d_copy_seconds", "d2h_copy_seconds")] + \
               [("h2d_bytes", C.c_uint64), ("d2h_bytes", C.c_uint64)]


SAM_SINK = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_size_t)
RG_HEADER = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.POINTER(C.c_int32))


class NativeAligner:
    """bmh_aligner_t: the native reads -> SAM pipeline; lanes (streams, workspaces, pinned staging) are kept between runs"""

    def __init__(self, index: "Index", pac: np.ndarray, l_pac: int, contigs, is_alt, copt, ep, po, pe):
        L = load_library()
        L.bmh_aligner_create.restype = C.c_void_p
        L.bmh_aligner_create.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.POINTER(C.c_char_p), C.c_void_p, C.c_void_p, C.POINTER(ChainOpt), C.POINTER(ExtParams),
                                         C.POINTER(PostOpt), C.POINTER(PeOpt)]
        L.bmh_aligner_free.argtypes = [C.c_void_p]
        run_tail = [C.c_int, C.c_int, C.c_int, SAM_SINK, C.c_void_p, C.POINTER(AlignStats)]      # paired, n_lanes, n_threads, sink, user, stats: the runs' common arguments
        for name, head in (("bmh_aligner_run", [C.POINTER(ReadSetT), C.c_void_p, C.c_uint32]), ("bmh_aligner_run_fasta", [C.c_char_p, C.c_uint64, C.c_uint64]),
                           ("bmh_aligner_run_file", [C.c_char_p, C.c_uint64, C.c_uint64]), ("bmh_aligner_run_files", [C.c_char_p, C.c_char_p, C.c_uint64, C.c_uint64])):
            getattr(L, name).restype = C.c_int
            getattr(L, name).argtypes = [C.c_void_p] + head + run_tail
        names = (C.c_char_p * len(contigs))(*[c[0].encode() for c in contigs])
        lens = np.ascontiguousarray([c[1] for c in contigs], dtype=np.int32)
        alt = np.ascontiguousarray(is_alt, dtype=np.uint8) if is_alt is not None else None
        self._pac = np.ascontiguousarray(pac, dtype=np.uint8)          # (borrowed by the handle: kept alive here)
        self._index = index
        self.options = (bytes(copt), bytes(ep), bytes(po), bytes(pe))  # what the handle was made with: the caller makes a new one when they change
        self.handle = L.bmh_aligner_create(index.handle, self._pac.ctypes.data, int(l_pac), len(contigs), names, lens.ctypes.data, alt.ctypes.data if alt is not None else None,
                                           C.byref(copt), C.byref(ep), C.byref(po), C.byref(pe))
        if not self.handle:
            raise RuntimeError("bmh_aligner_create: " + _err(L))

    def set_max_qlen(self, cap: int) -> None:
        """bmh_aligner_set_max_qlen: the extension cap of the runs that follow (768 by default, EXT_LONG_MAX for reads of any length)"""
        L = load_library()
        L.bmh_aligner_set_max_qlen.argtypes = [C.c_void_p, C.c_uint32]
        if L.bmh_aligner_set_max_qlen(self.handle, int(cap)) != 0:
            raise ValueError("bmh_aligner_set_max_qlen: " + _err(L))

    def set_reseed(self, opt: "ReseedOpt | None") -> None:
        """bmh_aligner_set_reseed: the seeding rounds of the runs that follow (None: re-seeding off)"""
        L = load_library()
        if L.bmh_aligner_set_reseed(self.handle, C.byref(opt) if opt is not None else None) != 0:
            raise ValueError("bmh_aligner_set_reseed: " + _err(L))

    def set_output(self, fmt: str = "sam", level: int = 1) -> None:
        """bmh_aligner_set_output: what the runs that follow hand to `write` -- "sam": the records' text; "bam": BGZF members of BAM records; "bam_sorted":
        set_sorted(level=level) with every other keyword at its default"""
        L = load_library()
        L.bmh_aligner_set_output.argtypes = [C.c_void_p, C.c_int, C.c_int]
        codes = {"sam": OUT_SAM, "bam": OUT_BAM, "bam_sorted": OUT_BAM_SORTED}      # ("bam_sorted": sorted runs, merged at the end of the input)
        if fmt not in codes or L.bmh_aligner_set_output(self.handle, codes[fmt], int(level)) != 0:
            raise ValueError("bmh_aligner_set_output: " + (_err(L) if fmt in codes else f"format {fmt!r} (sam or bam)"))

    def set_sorted(self, **keywords) -> None:
        """bmh_aligner_set_sorted_output: the runs that follow hand `write` the members of the coordinate-sorted file, made under sorted_request's keywords -- markdup,
        optical_distance, barcode_tag, barcode_name, barcode_edits, coverage, stats, index_format, csi_min_shift, level, window, sort_mem, sort_tmp (read_groups come
        from run_groups or set_keep_rg and are refused here).  Everything is checked before anything changes: a ValueError leaves the aligner as it was.  Any
        set_output switches all of it off again"""
        L = load_library()
        q = sorted_request("bmh_aligner_set_sorted_output", L, **keywords)
        L.bmh_aligner_set_sorted_output.argtypes = [C.c_void_p, C.POINTER(SortedOpt)]
        if L.bmh_aligner_set_sorted_output(self.handle, C.byref(q.opt)) != 0:
            raise ValueError("bmh_aligner_set_sorted_output: " + _err(L))
        self._sorted_req = q                                       # (a recalibration table's mask stays the caller's until the run is over: kept alive here)

    def sorted_results(self, *need) -> dict:
        """bmh_aligner_sorted_results: what the last sorted run left, each where the run computed it -- "markdup_counts" (MARKDUP_COUNTS' names), "markdup_library_counts"
        and "markdup_library_optical_counts" (a list, one dict per library of a run over read groups), "markdup_times" (decision_ms, window_flags_ms,
        entries_d2h_bytes), "markdup_barcode_counts", "markdup_barcode_group_counts", "markdup_optical_counts", "markdup_optical_ms", "coverage" (bam_coverage's
        arrays), "coverage_ms" ((device milliseconds, windows timed)), "stats" (bam_stats' arrays), "stats_ms".  need: names of SORTED_PARTS the caller insists on; a
        part the last run did not compute raises ValueError saying so"""
        L = load_library()
        L.bmh_aligner_sorted_results.argtypes = [C.c_void_p, C.POINTER(SortedResults), C.c_uint32]
        mask = 0
        for nm in need:
            mask |= SORTED_PARTS[nm]
        res = SortedResults()
        if L.bmh_aligner_sorted_results(self.handle, C.byref(res), mask) != 0:
            raise ValueError("bmh_aligner_sorted_results: " + _err(L))
        has = {nm for nm, bit in SORTED_PARTS.items() if res.parts & bit}
        n_lib = int(res.n_libraries)
        mc, cov, st, rt = MarkdupCounts(), Coverage(), BamStats(), Recal()
        rows, opt_rows = ((C.c_uint64 * (k * max(n_lib, 1)))() for k in (8, 3))
        mc.lib_counts, mc.lib_optical = C.cast(rows, _u64p), C.cast(opt_rows, _u64p)
        res = SortedResults(C.pointer(mc) if "markdup" in has else None, C.pointer(cov) if "coverage" in has else None, C.pointer(st) if "stats" in has else None)
        if "recal" in has:                                         # (the results' last members are read only under `need`)
            res.recal = C.pointer(rt); mask |= SORTED_PARTS["recal"]
        if L.bmh_aligner_sorted_results(self.handle, C.byref(res), mask) != 0:
            raise ValueError("bmh_aligner_sorted_results: " + _err(L))
        out = {}
        if "markdup" in has:
            out["markdup_counts"] = dict(zip(MARKDUP_COUNTS, (int(v) for v in mc.counts)))
            out["markdup_library_counts"] = [dict(zip(MARKDUP_COUNTS, (int(v) for v in rows[8 * k:8 * k + 8]))) for k in range(n_lib)]
            out["markdup_times"] = dict(decision_ms=res.markdup_ms[0], window_flags_ms=res.markdup_ms[1], entries_d2h_bytes=int(res.markdup_d2h_bytes))
        if "barcode" in has:
            out["markdup_barcode_counts"] = {"templates_without_barcode": int(mc.no_barcode)}
        if "grouped" in has:
            out["markdup_barcode_group_counts"] = dict(zip(BARCODE_GROUP_COUNTS, (int(v) for v in mc.grouped)))
        if "optical" in has:
            out["markdup_optical_counts"] = dict(zip(OPTICAL_COUNTS, (int(v) for v in mc.optical)))
            out["markdup_library_optical_counts"] = [dict(zip(OPTICAL_COUNTS, (int(v) for v in opt_rows[3 * k:3 * k + 3]))) for k in range(n_lib)]
            out["markdup_optical_ms"] = float(res.optical_ms)
        if "coverage" in has:
            out["coverage"], out["coverage_ms"] = coverage_dict(L, cov), (float(res.coverage_ms), int(res.coverage_windows))
        if "stats" in has:
            out["stats"], out["stats_ms"] = stats_dict(L, st), (float(res.stats_ms), int(res.stats_windows))
        if "recal" in has:
            kw = getattr(getattr(self, "_sorted_req", None), "recal_kw", {})
            out["recal"], out["recal_ms"] = recal_dict(L, rt, kw.get("read_groups"), kw.get("known_sites")), (float(res.recal_ms), int(res.recal_windows))
        return out

    def sort_index(self, base_offset: int) -> bytes:
        """bmh_aligner_sort_index: the .bai (or, for a run under index_format="csi", .csi) bytes of the last sorted run; base_offset: the bytes written before the sink's first (the header members)"""
        L = load_library()
        L.bmh_aligner_sort_index.argtypes = [C.c_void_p, C.c_uint64, C.POINTER(C.c_void_p), _u64p]
        L.bmh_free.argtypes = [C.c_void_p]
        out, n = C.c_void_p(), C.c_uint64()
        if L.bmh_aligner_sort_index(self.handle, int(base_offset), C.byref(out), C.byref(n)) != 0:
            raise ValueError("bmh_aligner_sort_index: " + _err(L))
        try:
            return C.string_at(out.value, n.value)
        finally:
            L.bmh_free(out)

    def host_tail_batches(self) -> int:
        """batches of the last run whose region tail the device refused (the host forms took them)"""
        L = load_library()
        L.bmh_aligner_host_tail_batches.restype = C.c_uint64
        L.bmh_aligner_host_tail_batches.argtypes = [C.c_void_p]
        return int(L.bmh_aligner_host_tail_batches(self.handle))

    def _run(self, name: str, args, write, bam_refusal: bool = True, read_errors=()) -> "AlignStats":
        """one run through the native entry point `name`: write(memoryview) receives every batch's records in order.  An exception of `write` is raised again after
        the run (it must not cross the C frames); else a return code raises BamRefusal (where bam_refusal), ReadFileError (a message with one of read_errors),
        CapacityError or RuntimeError"""
        L = load_library()
        err = []

        def sink(_user, ptr, n):
            try:
                write(memoryview((C.c_char * n).from_address(ptr)))
                return 0
            except BaseException as e:                      # noqa: BLE001 -- reported after the run
                err.append(e)
                return 1
        st = AlignStats()
        rc = getattr(L, name)(self.handle, *args, SAM_SINK(sink), None, C.byref(st))
        if err:
            raise err[0]
        if rc != 0:
            msg = _err(L)
            if bam_refusal and msg.startswith("BAM output:"):
                raise BamRefusal(msg)
            if any(m in msg for m in read_errors):
                raise ReadFileError(msg)
            raise (CapacityError if rc == -3 else RuntimeError)(f"{name} rc={rc}: " + msg)
        return st

    def run(self, rs, cuts, paired: bool, write, n_lanes: int = 2, n_threads: int = 0) -> "AlignStats":
        """the batches [cuts[b], cuts[b+1]) of the read set `rs` (an aligner.ReadSet; codes required); write(memoryview) receives every
        batch's SAM records in order"""
        keep = [np.ascontiguousarray(rs.ascii, dtype=np.uint8), np.ascontiguousarray(rs.codes, dtype=np.uint8), np.ascontiguousarray(rs.offs, dtype=np.uint64),
                np.ascontiguousarray(rs.lens, dtype=np.uint32), np.ascontiguousarray(rs.name_blob, dtype=np.uint8), np.ascontiguousarray(rs.name_off, dtype=np.uint64)]
        c = ReadSetT()
        c.n_reads = len(keep[3]); c.n_bases = int(keep[2][-1] + keep[3][-1]) if len(keep[3]) else 0; c.n_name_bytes = len(keep[4])
        c.ascii, c.codes, c.offs, c.lens, c.names, c.name_offs = (k.ctypes.data for k in keep)
        if getattr(rs, "qual", None) is not None:               # FASTQ: QUAL from these (same offsets as the letters)
            keep.append(np.ascontiguousarray(rs.qual, dtype=np.uint8)); c.quals = keep[-1].ctypes.data
        if getattr(rs, "comments", None) is not None:           # (blob, offsets): written with -C
            keep.append(np.ascontiguousarray(rs.comments[0], dtype=np.uint8)); c.comments = keep[-1].ctypes.data; c.n_comment_bytes = len(keep[-1])
            keep.append(np.ascontiguousarray(rs.comments[1], dtype=np.uint64)); c.comment_offs = keep[-1].ctypes.data
        cu = np.ascontiguousarray(cuts, dtype=np.uint64)
        return self._run("bmh_aligner_run", (C.byref(c), cu.ctypes.data, len(cu) - 1, 1 if paired else 0, int(n_lanes), int(n_threads)), write)

    def run_fasta(self, path: str, paired: bool, write, batch_bases: int = 0, batch_reads: int = 0, n_lanes: int = 2, n_threads: int = 0) -> "AlignStats":
        """bmh_aligner_run_fasta: the read file `path` batch by batch (cut by bases like the reference's bseq_read, or by reads), a loader thread ahead of the
        lanes; write(memoryview) receives every batch's SAM records in order"""
        return self._run("bmh_aligner_run_fasta", (path.encode(), int(batch_bases), int(batch_reads), 1 if paired else 0, int(n_lanes), int(n_threads)), write, bam_refusal=False)

    def run_file(self, path: str, paired: bool, write, batch_bases: int = 0, batch_reads: int = 0, n_lanes: int = 2, n_threads: int = 0) -> "AlignStats":
        """bmh_aligner_run_file: run_fasta for a FASTA or FASTQ file (QUAL from the qualities; the comments with -C)"""
        return self._run("bmh_aligner_run_file", (path.encode(), int(batch_bases), int(batch_reads), 1 if paired else 0, int(n_lanes), int(n_threads)), write,
                         read_errors=("FASTQ:", "reads file:"))

    def set_bam_pairs(self, batch_bases: int = 0, n_lanes: int = 0) -> None:
        """bmh_aligner_set_bam_pairs: the batch size and lanes run_files takes when its input turns out to be a BAM that holds pairs and paired was False"""
        L = load_library()
        L.bmh_aligner_set_bam_pairs.argtypes = [C.c_void_p, C.c_uint64, C.c_int]
        if L.bmh_aligner_set_bam_pairs(self.handle, int(batch_bases), int(n_lanes)) != 0:
            raise ValueError("bmh_aligner_set_bam_pairs: " + _err(L))

    def set_collate(self, on: bool, mem_bytes=None) -> None:
        """bmh_aligner_set_collate: run_files / run_groups find the mates of a BAM's pairs by name, in any record order; mem_bytes: the cap on the open records'
        bytes (None: the default of 8 GiB)"""
        L = load_library()
        L.bmh_aligner_set_collate.argtypes = [C.c_void_p, C.c_int, C.c_uint64]
        if L.bmh_aligner_set_collate(self.handle, 1 if on else 0, int(mem_bytes or 0)) != 0:
            raise ValueError("bmh_aligner_set_collate: " + _err(L))

    def set_keep_rg(self, on: bool, header=None) -> None:
        """bmh_aligner_set_keep_rg: run_files keeps the read groups of its input, one BAM.  header(lines, libraries) -- the @RG lines verbatim and every line's
        library index -- is called once the input's header has been read, before write() receives anything; an exception it raises ends the run and is raised
        again by run_files"""
        L = load_library()
        self._rg_err = []

        def cb(_user, ptr, n, ng, lib):
            try:
                header(C.string_at(ptr, n).decode("latin-1").split("\n")[:-1], [int(lib[k]) for k in range(ng)])
                return 0
            except BaseException as e:                      # noqa: BLE001 -- reported after the run
                self._rg_err.append(e)
                return 1
        self._rg_cb = RG_HEADER(cb) if on and header is not None else C.cast(None, RG_HEADER)      # (kept alive while the aligner may call it)
        L.bmh_aligner_set_keep_rg.argtypes = [C.c_void_p, C.c_int, RG_HEADER, C.c_void_p]
        if L.bmh_aligner_set_keep_rg(self.handle, 1 if on else 0, self._rg_cb, None) != 0:
            raise ValueError("bmh_aligner_set_keep_rg: " + _err(L))

    def run_files(self, path1: str, path2: str | None, paired: bool, write, batch_bases: int = 0, batch_reads: int = 0, n_lanes: int = 2, n_threads: int = 0) -> "AlignStats":
        """bmh_aligner_run_files: run_file for one or two read files of any shape (multi-line records, gzip / BGZF, pipes; path2: the mates)"""
        try:
            return self._run("bmh_aligner_run_files", (os.fsencode(path1), os.fsencode(path2) if path2 is not None else None, int(batch_bases), int(batch_reads),
                                                       1 if paired else 0, int(n_lanes), int(n_threads)), write, read_errors=("FASTQ:", "reads file", "bmh_aligner_run_files: the input's read groups"))
        except Exception:
            if getattr(self, "_rg_err", None):              # the header callback's own exception, not the library's account of it
                raise self._rg_err.pop()
            raise

    def run_groups(self, groups, paired: bool, write, batch_bases: int = 0, batch_reads: int = 0, n_lanes: int = 2, n_threads: int = 0) -> "AlignStats":
        """bmh_aligner_run_groups: run_files over several read groups in one run -- groups: [(id, library index, path1, path2 or None)]; every batch's records
        carry their group's ID.  What the library refuses of the groups or their files raises ReadFileError (a ValueError) naming the group"""
        L = load_library()
        g = (ReadGroupT * max(len(groups), 1))()
        for k, (rid, lib, p1, p2) in enumerate(groups):
            g[k].id = rid if isinstance(rid, bytes) else str(rid).encode(); g[k].library = int(lib)
            g[k].path1 = os.fsencode(p1); g[k].path2 = os.fsencode(p2) if p2 is not None else None
        L.bmh_aligner_run_groups.restype = C.c_int
        L.bmh_aligner_run_groups.argtypes = [C.c_void_p, C.POINTER(ReadGroupT), C.c_int, C.c_uint64, C.c_uint64, C.c_int, C.c_int, C.c_int, SAM_SINK, C.c_void_p, C.POINTER(AlignStats)]
        return self._run("bmh_aligner_run_groups", (g, len(groups), int(batch_bases), int(batch_reads), 1 if paired else 0, int(n_lanes), int(n_threads)), write,
                         read_errors=("FASTQ:", "reads file", "read group", "bmh_aligner_run_groups:"))

    def free(self):
        if self.handle:
            load_library().bmh_aligner_free(self.handle)
            self.handle = None


class ReseedOpt(C.Structure):
    """bmh_reseed_opt_t: BWA-MEM's second and third seeding rounds (gase_aln -g)"""
    _fields_ = [("enable", C.c_int), ("split_factor", C.c_float), ("split_width", C.c_int), ("max_mem_intv", C.c_int)]

    @classmethod
    def default(cls, **kw) -> "ReseedOpt":
        """mem_opt_init's values (re-seeding off, 1.5, 10, 20), then the keyword arguments (enable, split_factor, split_width, max_mem_intv)"""
        o = cls()
        load_library().bmh_reseed_opt_default(C.byref(o))
        for k, v in kw.items():
            if k not in ("enable", "split_factor", "split_width", "max_mem_intv"):
                raise TypeError(f"ReseedOpt: unknown field {k}")
            setattr(o, k, v)
        return o


class SeedsT(C.Structure):
    _fields_ = [("n_seeds", C.c_uint64), ("n_smems", C.c_uint64), ("n_cands", C.c_uint64),
                ("d_rbeg", C.c_void_p), ("d_qbeg", C.c_void_p), ("d_score", C.c_void_p),
                ("d_n_ref_pos", C.c_void_p), ("d_prefix", C.c_void_p)]


class ExtParams(C.Structure):
    """bmh_ext_params_t; defaults = the GPU pipeline's (src/bwamem.c:101-146)."""
    _fields_ = [(n, C.c_int) for n in ("a", "b", "o_del", "e_del", "o_ins", "e_ins", "zdrop", "end_bonus")]

    @classmethod
    def default(cls, zdrop: int = 0) -> "ExtParams":
        return cls(1, 4, 6, 1, 6, 1, zdrop, 5)


class ChainOpt(C.Structure):
    _fields_ = [(n, C.c_int) for n in ("a", "b", "o_del", "e_del", "o_ins", "e_ins", "w", "min_seed_len", "max_occ",
                                       "max_chain_gap", "min_chain_weight", "max_chain_extend")] + \
               [("mask_level", C.c_float), ("drop_ratio", C.c_float), ("contig_is_alt", C.c_void_p)]


class PostOpt(C.Structure):
    """bmh_post_opt_t"""
    _fields_ = [("T", C.c_int), ("mask_level_redun", C.c_float), ("mapQ_coef_len", C.c_float), ("mapQ_coef_fac", C.c_int),
                ("flag_all", C.c_int), ("id0", C.c_int64), ("XA_drop_ratio", C.c_float), ("max_XA_hits", C.c_int),
                ("no_multi", C.c_int), ("softclip", C.c_int), ("max_XA_hits_alt", C.c_int), ("contig_is_alt", C.c_void_p), ("rg_id", C.c_char_p),
                ("copy_comment", C.c_int)]


class PeOpt(C.Structure):
    """bmh_pe_opt_t"""
    _fields_ = [("pen_unpaired", C.c_int), ("max_ins", C.c_int), ("max_matesw", C.c_int), ("no_rescue", C.c_int), ("no_pairing", C.c_int)]


class BuildStats(C.Structure):
    """bmh_build_stats_t"""
    _fields_ = [("round0_passes", C.c_int), ("doubling_rounds", C.c_int), ("verified", C.c_int), ("unresolved_after_round0", C.c_uint64),
                ("round0_seconds", C.c_double), ("sa_seconds", C.c_double), ("verify_seconds", C.c_double), ("total_seconds", C.c_double)]


class DevJobsT(C.Structure):
    """bmh_dev_jobs_t"""
    _fields_ = [(n, C.c_uint64) for n in ("n_jobs", "n_regs", "q_bytes", "t_bytes", "n_heavy_reads")] + \
               [(n, C.c_void_p) for n in ("d_q", "d_qoff", "d_qlen", "d_t", "d_toff", "d_tlen", "d_h0", "d_job_read", "d_job_reg",
                                          "d_job_side", "d_regs_per_read", "d_frac_rep")]


# mirrors of include/seed_gen.h
class BwtTGpu(C.Structure):
    _fields_ = [("primary", C.c_uint64), ("L2", _u64p), ("seq_len", C.c_uint64), ("bwt_size", C.c_uint64),
                ("bwt", _u32p), ("sa_intv", C.c_int), ("n_sa", C.c_uint64), ("sa", _u32p),
                ("sa_upper_bits", _u32p), ("pack_size", C.c_uint8)]


class MemSeedVGpu(C.Structure):
    _fields_ = [("rbeg", _u64p), ("qbeg", _i32p), ("score", _u32p), ("n_ref_pos_fow_rev_results", _u32p),
                ("n_ref_pos_fow_rev_prefix_sums", _u32p), ("file_bytes_skip", C.c_uint64)]


class GpuseedStorageVector(C.Structure):
    _fields_ = [("read_file", C.c_char_p), ("query_file", C.c_char_p), ("bwt", C.POINTER(BwtTGpu)),
                ("bwt_gpu", BwtTGpu), ("pre_calc_seed_intervals", C.c_void_p),
                ("pre_calc_seed_intervals_flag", C.c_int), ("pre_calc_seed_len", C.c_int),
                ("min_seed_size", C.c_int), ("is_smem", C.c_int), ("file_bytes_skip", C.c_uint64)]


_LIB = None


def sources_sha16() -> str:
    """First 16 hex digits of the sha256 over the library's sources (csrc/*.hip, *.h, *.cpp and include/**/*.h, in name order):
    the build id a counter profile under profiles/ is stamped with (scripts/summarize_profiles.py) and bench.py compares
    before it quotes a counter from such a file."""
    import glob
    import hashlib
    here = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    root = os.path.dirname(here)
    files = sorted(glob.glob(os.path.join(here, "csrc", "*.hip")) + glob.glob(os.path.join(here, "csrc", "*.h")) + glob.glob(os.path.join(here, "csrc", "*.cpp")) +
                   glob.glob(os.path.join(root, "include", "**", "*.h"), recursive=True))
    h = hashlib.sha256()
    for f in files:
        h.update(os.path.relpath(f, root).encode() + b"\0")
        h.update(open(f, "rb").read())
    return h.hexdigest()[:16]


def load_library() -> C.CDLL:
    """Load libbwamem_hip.so; raises HipLibraryMissing (never falls back) if it is not built."""
    global _LIB
    if _LIB is not None:
        return _LIB
    p = lib_path()
    if not os.path.exists(p):
        raise HipLibraryMissing(f"{p} not found: build it with `make -C bwa-mem_gpu_amd/csrc` "
                                "(or __graft_entry__.build()); there is no CPU fallback")
    L = C.CDLL(p)
    L.bmh_last_error.restype = C.c_char_p
    L.bmh_device_count.restype = C.c_int
    L.bmh_set_device.argtypes = [C.c_int]
    L.bmh_index_upload.restype = C.c_void_p
    L.bmh_index_upload.argtypes = [C.c_uint64, _u64p, C.c_uint64, _u32p, C.c_uint64, C.c_int, _u32p, C.c_uint64,
                                   _u32p, _u8p, C.c_uint64]
    L.bmh_index_from_device.restype = C.c_void_p
    L.bmh_index_from_device.argtypes = [C.c_uint64, _u64p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_int, C.c_void_p,
                                        C.c_uint64, C.c_void_p, C.c_void_p, C.c_uint64]
    L.bmh_index_free.argtypes = [C.c_void_p]
    L.bmh_index_kbits_info.restype = C.c_int
    L.bmh_index_kbits_info.argtypes = [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_void_p), _u64p]
    L.bmh_tune_set.restype = C.c_int
    L.bmh_wtrace_start.restype = C.c_int
    L.bmh_wtrace_start.argtypes = [C.c_uint32]
    L.bmh_wtrace_stop.restype = C.c_int64
    L.bmh_wtrace_stop.argtypes = [C.c_void_p, C.c_uint32]
    L.bmh_wtrace_kept.restype = C.c_uint32
    L.bmh_tune_set.argtypes = [C.c_char_p, C.c_int, C.c_int]
    L.bmh_rccl_where.restype = C.c_char_p
    L.bmh_rccl_unique_id.restype = C.c_int
    L.bmh_rccl_unique_id.argtypes = [C.c_void_p]
    L.bmh_rccl_comm_init_rank.restype = C.c_int
    L.bmh_rccl_comm_init_rank.argtypes = [C.POINTER(C.c_void_p), C.c_int, C.c_void_p, C.c_int]
    L.bmh_rccl_comm_destroy.argtypes = [C.c_void_p]
    L.bmh_index_broadcast_rccl.restype = C.c_int
    L.bmh_index_broadcast_rccl.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.POINTER(C.c_void_p), C.c_void_p]
    L.bmh_index_replicate_all.restype = C.c_int
    L.bmh_index_replicate_all.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_int), C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_int)]
    L.bmh_index_probe.restype = C.c_int
    L.bmh_index_probe.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_int, C.c_void_p, C.c_void_p]
    L.bmh_index_densify_sa.restype = C.c_int
    L.bmh_index_densify_sa.argtypes = [C.c_void_p, C.c_int]
    L.bmh_index_build.restype = C.c_int
    L.bmh_index_build.argtypes = [C.c_void_p, C.c_uint64, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, _u64p, _u64p, C.c_int, C.POINTER(BuildStats)]
    L.bmh_seed_ws_create.restype = C.c_void_p
    L.bmh_seed_ws_create.argtypes = [C.c_uint32, C.c_uint64, C.c_uint64, C.c_uint64]
    L.bmh_seed_ws_free.argtypes = [C.c_void_p]
    L.bmh_seed_batch.restype = C.c_int
    L.bmh_seed_batch.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_int,
                                 C.c_void_p, C.POINTER(SeedsT)]
    L.bmh_seed_last_timing.argtypes = [C.c_void_p, C.POINTER(C.c_float)]
    L.bmh_seed_ws_set_sample.restype = C.c_int
    L.bmh_seed_ws_set_sample.argtypes = [C.c_void_p, C.c_uint32]
    L.bmh_seeds_sample_state.restype = C.c_uint32
    L.bmh_seeds_sample_state.argtypes = [C.c_void_p]
    L.bmh_seeds_locate_all.restype = C.c_int
    L.bmh_seeds_locate_all.argtypes = [C.c_void_p, C.c_void_p]
    L.bmh_reseed_opt_default.argtypes = [C.POINTER(ReseedOpt)]
    L.bmh_seed_batch_reseed.restype = C.c_int
    L.bmh_seed_batch_reseed.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_int,
                                        C.POINTER(ReseedOpt), C.c_void_p, C.POINTER(SeedsT)]
    L.bmh_reseed_last_counts.restype = C.c_int
    L.bmh_reseed_last_counts.argtypes = [C.POINTER(C.c_uint64)]
    L.bmh_aligner_set_reseed.restype = C.c_int
    L.bmh_aligner_set_reseed.argtypes = [C.c_void_p, C.POINTER(ReseedOpt)]
    L.bmh_extend_batch.restype = C.c_int
    L.bmh_extend_batch.argtypes = [C.c_void_p] * 7 + [C.c_uint32, C.POINTER(ExtParams), C.c_void_p, C.c_void_p, C.c_void_p]
    L.bmh_extend_batch_long.restype = C.c_int
    L.bmh_extend_batch_long.argtypes = [C.c_void_p] * 7 + [C.c_uint32, C.POINTER(ExtParams), C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p]
    L.bmh_extend_last_ms.restype = C.c_float
    L.bmh_extend_last_unsupported.restype = C.c_int64
    L.bmh_extend_last_class_sizes.restype = C.c_int
    L.bmh_extend_last_class_sizes.argtypes = [C.c_void_p, C.c_int]
    L.bmh_calib_gather.restype = C.c_int
    L.bmh_calib_gather.argtypes = [C.c_void_p, C.c_uint64, C.c_int, C.c_int, C.c_void_p, C.POINTER(C.c_float)]
    L.bmh_calib_valu.restype = C.c_int
    L.bmh_calib_valu.argtypes = [C.c_int, C.c_int, C.c_int, C.c_void_p, C.POINTER(C.c_float), C.POINTER(C.c_double)]
    L.bmh_calib_valu_placed.restype = C.c_int
    L.bmh_calib_valu_placed.argtypes = [C.c_int, C.c_int, C.c_int, C.c_void_p, C.POINTER(C.c_float), C.POINTER(C.c_double), C.c_void_p, C.POINTER(C.c_uint)]
    L.bmh_chain_opt_default.argtypes = [C.POINTER(ChainOpt)]
    L.bmh_build_jobs.restype = C.c_void_p
    L.bmh_build_jobs.argtypes = [C.POINTER(ChainOpt), C.c_int64, _u8p, C.c_int, C.c_void_p, C.c_void_p, C.c_uint32, _u8p, _u64p, _u32p,
                                 _u64p, _i32p, _u32p, _u32p, _u32p, C.c_int]
    L.bmh_jobs_free.argtypes = [C.c_void_p]
    L.bmh_jobs_sizes.argtypes = [C.c_void_p, _u64p, _u64p, _u64p, _u64p]
    L.bmh_jobs_arrays.argtypes = [C.c_void_p] + [C.POINTER(C.c_void_p)] * 11
    L.bmh_jobs_frac_rep.restype = C.POINTER(C.c_float)
    L.bmh_jobs_frac_rep.argtypes = [C.c_void_p]
    L.bmh_post_opt_default.argtypes = [C.POINTER(PostOpt)]
    L.bmh_finalize_regs.restype = C.c_int64
    L.bmh_finalize_regs.argtypes = [C.POINTER(ChainOpt), C.POINTER(ExtParams), C.POINTER(PostOpt), C.c_int64, _u8p, C.c_uint32, _u8p, _u64p,
                                    _i32p, _u32p, C.POINTER(C.c_float), C.c_int, C.c_void_p, _i32p, _u32p, C.c_int]
    L.bmh_finalize_regs_device.restype = C.c_int64
    L.bmh_finalize_regs_device.argtypes = [C.c_void_p, C.POINTER(ChainOpt), C.POINTER(ExtParams), C.POINTER(PostOpt), C.c_void_p, C.c_void_p, C.c_uint32,
                                           C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.bmh_finalize_regs_device_last_ms.restype = C.c_float
    L.bmh_finalize_regs_device_last_classes.restype = C.c_int
    L.bmh_finalize_regs_device_last_classes.argtypes = [_u32p]
    L.bmh_sam_need_cigar.restype = C.c_int64
    L.bmh_sam_need_cigar.argtypes = [C.POINTER(PostOpt), _i32p, _u32p, C.c_uint32, _u8p]
    L.bmh_format_sam.restype = C.c_void_p
    L.bmh_format_sam.argtypes = [C.POINTER(PostOpt), C.c_uint32, C.c_void_p, _u64p, _u8p, _u64p, _u32p, C.c_int, C.POINTER(C.c_char_p), C.c_void_p,
                                 _i32p, _u32p, C.c_void_p, _i32p, _u32p, C.c_int, C.c_void_p, C.c_int, C.POINTER(C.c_size_t)]
    L.bmh_free.argtypes = [C.c_void_p]
    L.bmh_pe_opt_default.argtypes = [C.POINTER(PeOpt)]
    L.bmh_finalize_pairs.restype = C.c_int64
    L.bmh_finalize_pairs.argtypes = [C.POINTER(ChainOpt), C.POINTER(ExtParams), C.POINTER(PostOpt), C.POINTER(PeOpt), C.c_int64, _u8p, C.c_uint32, _u8p, _u64p,
                                     _u32p, _i32p, _u32p, C.POINTER(C.c_float), C.c_int, C.c_void_p, C.c_void_p, _i32p, C.c_uint64, _u32p, _i32p, _i32p,
                                     C.c_void_p, C.c_int]
    L.bmh_finalize_pairs_dev.restype = C.c_int64
    L.bmh_finalize_pairs_dev.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p] + list(L.bmh_finalize_pairs.argtypes)
    L.bmh_rescue_check_counts.restype = None
    L.bmh_rescue_check_counts.argtypes = [C.POINTER(C.c_uint64)]
    L.bmh_finalize_pairs_deduped.restype = C.c_int64
    L.bmh_finalize_pairs_deduped.argtypes = list(L.bmh_finalize_pairs_dev.argtypes)
    L.bmh_dedup_regs_device.restype = C.c_int64
    L.bmh_dedup_regs_device.argtypes = [C.c_void_p, C.POINTER(ChainOpt), C.POINTER(ExtParams), C.POINTER(PostOpt), C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint64, C.c_void_p,
                                        C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.bmh_sam_need_cigar_pe.restype = C.c_int64
    L.bmh_sam_need_cigar_pe.argtypes = [C.POINTER(PostOpt), _i32p, _u32p, _i32p, C.c_uint32, _u8p]
    L.bmh_format_sam_pe.restype = C.c_void_p
    L.bmh_format_sam_pe.argtypes = [C.POINTER(PostOpt), C.c_uint32, C.c_void_p, _u64p, _u8p, _u64p, _u32p, C.c_int, C.POINTER(C.c_char_p), C.c_void_p,
                                    _i32p, _u32p, _i32p, _i32p, C.c_void_p, _i32p, _u32p, C.c_int, C.c_void_p, C.c_int, C.POINTER(C.c_size_t)]
    L.bmh_format_sam_ex.restype = C.c_void_p
    L.bmh_format_sam_ex.argtypes = [C.POINTER(PostOpt), C.c_uint32, C.c_void_p, _u64p, _u8p, _u64p, _u32p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int,
                                    C.POINTER(C.c_char_p), C.c_void_p, _i32p, _u32p, C.c_void_p, _i32p, _u32p, C.c_int, C.c_void_p, C.c_int, C.POINTER(C.c_size_t)]
    L.bmh_format_sam_pe_ex.restype = C.c_void_p
    L.bmh_format_sam_pe_ex.argtypes = [C.POINTER(PostOpt), C.c_uint32, C.c_void_p, _u64p, _u8p, _u64p, _u32p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int,
                                       C.POINTER(C.c_char_p), C.c_void_p, _i32p, _u32p, _i32p, _i32p, C.c_void_p, _i32p, _u32p, C.c_int, C.c_void_p, C.c_int,
                                       C.POINTER(C.c_size_t)]
    L.bmh_format_sam_groups.restype = C.c_void_p
    L.bmh_format_sam_groups.argtypes = [C.POINTER(PostOpt), C.c_uint32, C.c_void_p, _u64p, _u8p, _u64p, _u32p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int,
                                        C.POINTER(C.c_char_p), C.c_void_p, _i32p, _u32p, C.c_void_p, C.c_void_p, C.c_void_p, _i32p, _u32p, C.c_int, C.c_void_p, C.c_int,
                                        C.POINTER(ReadGroupsT), C.POINTER(C.c_size_t)]
    L.bmh_merge_regs.restype = C.c_int
    L.bmh_merge_regs.argtypes = [C.c_void_p, _i32p, _i32p]
    L.bmh_chain_ws_create.restype = C.c_void_p
    L.bmh_chain_ws_create.argtypes = [C.c_uint32, C.c_uint64]
    L.bmh_chain_ws_free.argtypes = [C.c_void_p]
    L.bmh_chain_set_contigs.restype = C.c_int
    L.bmh_chain_set_contigs.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
    L.bmh_chain_set_alt.restype = C.c_int
    L.bmh_chain_set_alt.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
    L.bmh_chain_batch.restype = C.c_int
    L.bmh_chain_batch.argtypes = [C.c_void_p, C.POINTER(ChainOpt), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32,
                                  C.POINTER(SeedsT), C.c_void_p, C.POINTER(DevJobsT)]
    L.bmh_chain_set_materialize.restype = C.c_int
    L.bmh_chain_set_materialize.argtypes = [C.c_void_p, C.c_int]
    L.bmh_chain_extend.restype = C.c_int
    L.bmh_chain_extend.argtypes = [C.c_void_p, C.POINTER(ExtParams), C.c_void_p, C.c_void_p, C.c_void_p]
    L.bmh_chain_extend_merge.restype = C.c_int
    L.bmh_chain_extend_merge.argtypes = [C.c_void_p, C.POINTER(ChainOpt), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32,
                                         C.POINTER(SeedsT), C.POINTER(ExtParams), C.c_void_p, C.c_uint64, C.c_void_p, C.POINTER(DevJobsT)]
    L.bmh_chain_extend_merge_timing.restype = C.c_int
    L.bmh_chain_extend_merge_timing.argtypes = [C.c_void_p, C.POINTER(C.c_float), _u64p]
    L.bmh_chain_last_timing.argtypes = [C.c_void_p, C.POINTER(C.c_float)]
    L.bmh_chain_class_counts.restype = C.c_int
    L.bmh_chain_class_counts.argtypes = [C.c_void_p, _u32p]
    L.bmh_chain_merge.restype = C.c_int
    L.bmh_chain_merge.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.bmh_cigar_batch.restype = C.c_int
    L.bmh_cigar_batch.argtypes = [C.c_void_p] * 5 + [C.c_int, C.c_void_p, C.c_uint32, C.POINTER(ExtParams), C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                                  C.c_int, C.c_void_p, C.c_void_p]
    L.bmh_cigar_release.restype = None
    L.bmh_cigar_release.argtypes = [C.c_void_p]
    L.bmh_sam_select_work.restype = C.c_size_t
    L.bmh_sam_select_work.argtypes = [C.c_uint32, C.c_uint64]
    L.bmh_sam_select_device.restype = C.c_int64
    L.bmh_sam_select_device.argtypes = [C.POINTER(PostOpt), C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
    L.bmh_cigar_pack_work.restype = C.c_size_t
    L.bmh_cigar_pack_work.argtypes = [C.c_uint32]
    L.bmh_cigar_pack_sizes.restype = C.c_int64
    L.bmh_cigar_pack_sizes.argtypes = [C.c_void_p, C.c_uint32, C.c_int, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
    L.bmh_cigar_pack.restype = C.c_int
    L.bmh_cigar_pack.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p]
    L.bmh_sam_text_work.restype = C.c_size_t
    L.bmh_sam_text_work.argtypes = [C.c_uint32]
    L.bmh_sam_text_sizes.restype = C.c_int64
    L.bmh_sam_text_sizes.argtypes = [C.POINTER(PostOpt), C.POINTER(SamDev), C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
    L.bmh_sam_text_write.restype = C.c_int
    L.bmh_sam_text_write.argtypes = [C.POINTER(PostOpt), C.POINTER(SamDev), C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
    L.bmh_sam_text_check.restype = C.c_int
    L.bmh_sam_text_check.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p]
    L.bwt_restore_bwt_gpu.restype = C.POINTER(BwtTGpu)
    L.bwt_restore_bwt_gpu.argtypes = [C.c_char_p]
    L.bwt_restore_sa_gpu.argtypes = [C.c_char_p, C.POINTER(BwtTGpu)]
    L.gpu_cpy_wrapper.restype = BwtTGpu
    L.gpu_cpy_wrapper.argtypes = [C.POINTER(BwtTGpu)]
    L.seed_gpu.restype = C.POINTER(MemSeedVGpu)
    L.seed_gpu.argtypes = [C.POINTER(GpuseedStorageVector)]
    L.free_gpuseed_data.argtypes = [C.POINTER(GpuseedStorageVector)]
    L.seed_gpu_last_n_reads.restype = C.c_uint64
    _LIB = L
    return L


def _err(L) -> str:
    return (L.bmh_last_error() or b"").decode()


def _np_ptr(a, t):
    return a.ctypes.data_as(t)


class Index:
    """FMD index resident in HBM (bmh_index_t)."""

    def __init__(self, handle, keep=None):
        self.handle = handle
        self._keep = keep

    @classmethod
    def upload(cls, idx, pac: np.ndarray | None = None, l_pac: int = 0) -> "Index":
        """idx: fmindex.FMDIndex on the host -> HBM (replaces gpu_cpy_wrapper)."""
        L = load_library()
        L2 = np.ascontiguousarray(idx.L2, dtype=np.uint64)
        bw = np.ascontiguousarray(idx.bwt_words, dtype=np.uint32)
        sa = np.ascontiguousarray(idx.sa, dtype=np.uint32)
        bits = np.ascontiguousarray(idx.sa_bits, dtype=np.uint32)
        h = L.bmh_index_upload(idx.primary, _np_ptr(L2, _u64p), idx.seq_len, _np_ptr(bw, _u32p), bw.shape[0],
                               idx.sa_intv, _np_ptr(sa, _u32p), idx.n_sa, _np_ptr(bits, _u32p),
                               _np_ptr(pac, _u8p) if pac is not None else None, l_pac)
        if not h:
            raise RuntimeError("bmh_index_upload: " + _err(L))
        return cls(h)

    @classmethod
    def from_device(cls, primary, L2, seq_len, bwt_t, sa_intv, sa_t, sa_bits_t, pac_t=None, l_pac=0) -> "Index":
        """Wrap torch tensors already in HBM (e.g. after the RCCL broadcast); tensors are kept alive."""
        L = load_library()
        L2a = np.ascontiguousarray(L2, dtype=np.uint64)
        h = L.bmh_index_from_device(primary, _np_ptr(L2a, _u64p), seq_len, bwt_t.data_ptr(), bwt_t.numel(), sa_intv,
                                    sa_t.data_ptr(), sa_t.numel(), sa_bits_t.data_ptr(),
                                    pac_t.data_ptr() if pac_t is not None else None, l_pac)
        if not h:
            raise RuntimeError("bmh_index_from_device: " + _err(L))
        return cls(h, keep=(bwt_t, sa_t, sa_bits_t, pac_t))

    def densify_sa(self, new_intv: int) -> None:
        """bmh_index_densify_sa: suffix-array samples of every new_intv-th row, computed on the device from the existing ones"""
        L = load_library()
        rc = L.bmh_index_densify_sa(self.handle, int(new_intv))
        if rc != 0:
            raise RuntimeError(f"bmh_index_densify_sa rc={rc}: " + _err(L))

    def probe(self, rows, what: str) -> np.ndarray:
        """bmh_index_probe: 'occ4' -> [n, 4] Occ counts, 'lf' -> LF(row), 'sa' -> SA[row] at the given rows (u64)"""
        import torch
        L = load_library()
        r = torch.from_numpy(np.ascontiguousarray(rows, dtype=np.uint64).view(np.int64)).cuda()
        code = {"occ4": 0, "lf": 1, "sa": 2}[what]
        out = torch.empty(r.numel() * (4 if code == 0 else 1), dtype=torch.int64, device="cuda")
        rc = L.bmh_index_probe(self.handle, r.data_ptr(), r.numel(), code, out.data_ptr(), torch.cuda.current_stream().cuda_stream)
        if rc != 0:
            raise RuntimeError(f"bmh_index_probe rc={rc}: " + _err(L))
        torch.cuda.synchronize()
        o = out.cpu().numpy().view(np.uint64)
        return o.reshape(-1, 4) if code == 0 else o

    def kbits_info(self) -> tuple:
        """bmh_index_kbits_info: (K, device pointer, 32-bit words) of the handle's K-mer bitmap; (0, 0, 0) when it has none"""
        L = load_library()
        k, p, n = C.c_int(0), C.c_void_p(None), C.c_uint64(0)
        rc = L.bmh_index_kbits_info(self.handle, C.byref(k), C.byref(p), C.byref(n))
        if rc != 0:
            raise RuntimeError(f"bmh_index_kbits_info rc={rc}: " + _err(L))
        return int(k.value), int(p.value or 0), int(n.value)

    def kbits_to_host(self) -> np.ndarray:
        """the K-mer bitmap's 32-bit words (test helper; uses torch only to read HBM); empty when the handle has none"""
        import torch
        _, p, n = self.kbits_info()
        if not n:
            return np.zeros(0, np.uint32)
        buf = torch.empty(n, dtype=torch.int32, device="cuda")
        _memcpy_d2d(buf.data_ptr(), p, n * 4)
        return buf.cpu().numpy().view(np.uint32)

    def free(self):
        if self.handle:
            load_library().bmh_index_free(self.handle)
            self.handle = None


class SeedWorkspace:
    def __init__(self, max_reads: int, max_bases: int, max_cands: int = 0, max_occ: int = 0, sample_max_occ: int = 500):
        """sample_max_occ: bmh_seed_ws_set_sample -- of an SMEM with more occurrences only those are located that chaining with this max_occ reads (500: BWA's
        default, what bmh_chain_opt_default sets); 0: every occurrence.  The chaining calls and seeds_to_host complete a sampled batch where they need more."""
        L = load_library()
        self.handle = L.bmh_seed_ws_create(max_reads, max_bases, max_cands, max_occ)
        if not self.handle:
            raise RuntimeError("bmh_seed_ws_create: " + _err(L))
        if L.bmh_seed_ws_set_sample(self.handle, int(sample_max_occ)) != 0:
            raise RuntimeError("bmh_seed_ws_set_sample: " + _err(L))

    def seed_batch(self, index: Index, reads_t, offs_t, lens_t, min_seed_len: int = 19, stream: int = 0, reseed: "ReseedOpt | None" = None) -> SeedsT:
        """reads_t/offs_t/lens_t: torch CUDA tensors (uint8 ASCII, int32/uint32 offsets and lengths).  reseed: a ReseedOpt with enable = 1 adds
        BWA-MEM's second and third seeding rounds (bmh_seed_batch_reseed); None or enable = 0: bmh_seed_batch."""
        L = load_library()
        out = SeedsT()
        if reseed is not None and reseed.enable:
            rc = L.bmh_seed_batch_reseed(self.handle, index.handle, reads_t.data_ptr(), offs_t.data_ptr(), lens_t.data_ptr(),
                                         lens_t.numel(), min_seed_len, C.byref(reseed), stream, C.byref(out))
        else:
            rc = L.bmh_seed_batch(self.handle, index.handle, reads_t.data_ptr(), offs_t.data_ptr(), lens_t.data_ptr(),
                                  lens_t.numel(), min_seed_len, stream, C.byref(out))
        if rc != 0:
            raise RuntimeError(f"bmh_seed_batch rc={rc}: " + _err(L))
        return out

    def timing(self):
        ms = (C.c_float * 7)()
        load_library().bmh_seed_last_timing(self.handle, ms)
        names = ("pack", "smem", "sort", "gather_scan", "expand", "locate", "total") if os.environ.get("BMH_SEED_FUSED") else ("pack", "forward", "backward", "filter_scan", "expand", "locate", "total")
        return dict(zip(names, list(ms)))

    def free(self):
        if self.handle:
            load_library().bmh_seed_ws_free(self.handle)
            self.handle = None


class ChainWorkspace:
    """Device job builder (bmh_chain_batch / bmh_chain_merge): seeds in HBM -> extension jobs in HBM -> regions."""

    def __init__(self, max_reads: int, max_seeds: int, opt: "ChainOpt | None" = None):
        L = load_library()
        self.handle = L.bmh_chain_ws_create(max_reads, max_seeds)
        if not self.handle:
            raise RuntimeError("bmh_chain_ws_create: " + _err(L))
        self.opt = opt or ChainOpt()
        if opt is None:
            L.bmh_chain_opt_default(C.byref(self.opt))

    def set_contigs(self, contigs) -> None:
        """contigs: list of (name, length) of the packed reference's sequences (bmh_chain_set_contigs)"""
        L = load_library()
        ln = np.ascontiguousarray([c[1] for c in contigs], dtype=np.int32)
        off = np.ascontiguousarray(np.concatenate([[0], np.cumsum(ln)[:-1]]), dtype=np.int64)
        rc = L.bmh_chain_set_contigs(self.handle, len(contigs), off.ctypes.data_as(C.c_void_p), ln.ctypes.data_as(C.c_void_p))
        if rc != 0:
            raise RuntimeError("bmh_chain_set_contigs: " + _err(L))

    def set_alt(self, is_alt) -> None:
        """is_alt: one flag per sequence of set_contigs' table (bmh_chain_set_alt; the .alt file of the index)"""
        L = load_library()
        a = np.ascontiguousarray(is_alt, dtype=np.uint8)
        rc = L.bmh_chain_set_alt(self.handle, len(a), a.ctypes.data_as(C.c_void_p))
        if rc != 0:
            raise RuntimeError("bmh_chain_set_alt: " + _err(L))

    def chain_batch(self, index: Index, reads_t, offs_t, lens_t, seeds: SeedsT, stream: int = 0) -> DevJobsT:
        L = load_library()
        out = DevJobsT()
        rc = L.bmh_chain_batch(self.handle, C.byref(self.opt), index.handle, reads_t.data_ptr(), offs_t.data_ptr(), lens_t.data_ptr(),
                               lens_t.numel(), C.byref(seeds), stream, C.byref(out))
        if rc != 0:
            raise RuntimeError(f"bmh_chain_batch rc={rc}: " + _err(L))
        self.last_jobs = out
        return out

    def set_materialize(self, on: bool) -> None:
        load_library().bmh_chain_set_materialize(self.handle, 1 if on else 0)

    def set_max_qlen(self, cap: int) -> None:
        """bmh_chain_ws_set_max_qlen: extend / extend_merge send query sides of 769 .. cap bases to the long-query classes (default 768: none);
        a batch with a longer one raises, naming the cap"""
        L = load_library()
        L.bmh_chain_ws_set_max_qlen.argtypes = [C.c_void_p, C.c_uint32]
        if L.bmh_chain_ws_set_max_qlen(self.handle, int(cap)) != 0:
            raise ValueError("bmh_chain_ws_set_max_qlen: " + _err(L))

    def extend(self, out3_t, params: "ExtParams | None" = None, raw_t=None, stream: int = 0) -> None:
        """bmh_chain_extend: extension of the last chain_batch's jobs straight from their descriptors."""
        L = load_library()
        p = params or ExtParams.default()
        rc = L.bmh_chain_extend(self.handle, C.byref(p), out3_t.data_ptr(), raw_t.data_ptr() if raw_t is not None else None, stream)
        if rc != 0:
            raise RuntimeError(f"bmh_chain_extend rc={rc}: " + _err(L))

    def extend_merge(self, index: Index, reads_t, offs_t, lens_t, seeds: SeedsT, regs_t, params: "ExtParams | None" = None, stream: int = 0) -> DevJobsT:
        """bmh_chain_extend_merge: chaining, extension and region merge of one batch in one call (regs_t int32 [cap, 8], read order)"""
        L = load_library()
        out = DevJobsT()
        p = params or ExtParams.default()
        rc = L.bmh_chain_extend_merge(self.handle, C.byref(self.opt), index.handle, reads_t.data_ptr(), offs_t.data_ptr(), lens_t.data_ptr(),
                                      lens_t.numel(), C.byref(seeds), C.byref(p), regs_t.data_ptr(), int(regs_t.shape[0]), stream, C.byref(out))
        if rc != 0:
            raise RuntimeError(f"bmh_chain_extend_merge rc={rc}: " + _err(L))
        self.last_jobs = out
        return out

    def extend_merge_timing(self):
        L = load_library()
        ms = (C.c_float * 3)(); jobs = (C.c_uint64 * 2)()
        L.bmh_chain_extend_merge_timing(self.handle, ms, jobs)
        return {"extend_a": ms[0], "extend_b": ms[1], "stage": ms[2], "jobs_a": int(jobs[0]), "jobs_b": int(jobs[1])}

    def timing(self):
        ms = (C.c_float * 8)()
        load_library().bmh_chain_last_timing(self.handle, ms)
        return {"classify": ms[0], "lane": ms[1], "wave": ms[2], "to_counts": ms[3], "reads_small_scratch": int(ms[6]), "reads_large_scratch": int(ms[7])}

    def class_counts(self) -> np.ndarray:
        """bmh_chain_class_counts: which form chained how many reads of the last batch -- [0..11) the size classes of the cooperative kernels,
        [11..15) the need bins of the lane kernel, [15] the reads of the long-read kernel"""
        L = load_library()
        out = np.zeros(16, np.uint32)
        if L.bmh_chain_class_counts(self.handle, _np_ptr(out, _u32p)) != 0:
            raise RuntimeError("bmh_chain_class_counts: " + _err(L))
        return out

    def merge(self, out3_t, regs_t, stream: int = 0) -> None:
        L = load_library()
        rc = L.bmh_chain_merge(self.handle, out3_t.data_ptr(), regs_t.data_ptr(), stream)
        if rc != 0:
            raise RuntimeError(f"bmh_chain_merge rc={rc}: " + _err(L))

    def free(self):
        if self.handle:
            load_library().bmh_chain_ws_free(self.handle)
            self.handle = None


def cigar_batch(index: Index, reads_t, offs_t, lens_t, regs_t, n: int, sel_t=None, params: "ExtParams | None" = None, opt_w: int = 300,
                max_cigar: int = 32, md_cap: int = 128, stream: int = 0):
    """bmh_cigar_batch on torch CUDA tensors; returns (cigar uint32 [n, max_cigar], aln int32 [n, 8], md uint8 [n, md_cap]) tensors."""
    import torch
    L = load_library()
    p = params or ExtParams.default()
    dev = regs_t.device
    cigar = torch.zeros(max(n, 1), max_cigar, dtype=torch.int32, device=dev)
    aln = torch.zeros(max(n, 1), 8, dtype=torch.int32, device=dev)
    md = torch.zeros(max(n, 1), md_cap, dtype=torch.uint8, device=dev)
    rc = L.bmh_cigar_batch(index.handle, reads_t.data_ptr(), offs_t.data_ptr(), lens_t.data_ptr(), regs_t.data_ptr(), int(regs_t.shape[1]),
                           sel_t.data_ptr() if sel_t is not None else None, n, C.byref(p), opt_w, max_cigar, cigar.data_ptr(), aln.data_ptr(),
                           md_cap, md.data_ptr(), stream)
    if rc != 0:
        raise RuntimeError(f"bmh_cigar_batch rc={rc}: " + _err(L))
    return cigar, aln, md


def sam_select_device(po: "PostOpt", fin_t, fin_per_read_t, h_rec_t=None, stream: int = 0):
    """bmh_sam_select_device on torch CUDA tensors (fin int32 [m, 16], fin_per_read int32 [n_reads], h_rec int32 [n_reads] for pairs):
    returns (sel int32 [n_sel], slot int32 [m]) on the device."""
    import torch
    L = load_library()
    m, n_reads = int(fin_t.shape[0]), int(fin_per_read_t.shape[0])
    dev = fin_t.device
    sel = torch.empty(max(m, 1), dtype=torch.int32, device=dev); slot = torch.empty(max(m, 1), dtype=torch.int32, device=dev)
    wb = int(L.bmh_sam_select_work(n_reads, m))
    work = torch.empty(wb, dtype=torch.uint8, device=dev)
    k = L.bmh_sam_select_device(C.byref(po), fin_t.data_ptr(), fin_per_read_t.data_ptr(), h_rec_t.data_ptr() if h_rec_t is not None else None, n_reads, m,
                                sel.data_ptr(), slot.data_ptr(), work.data_ptr(), wb, stream)
    if k < 0:
        raise RuntimeError(f"bmh_sam_select_device rc={k}: " + _err(L))
    return sel[:k], slot[:m]


def cigar_pack(aln_t, cigar_t, md_t=None, stream: int = 0):
    """bmh_cigar_pack_sizes + bmh_cigar_pack on the outputs of cigar_batch: returns (off int32 [n + 1], packed int32 [words]) on the device"""
    import torch
    L = load_library()
    n = int(aln_t.shape[0])
    dev = aln_t.device
    off = torch.empty(n + 2, dtype=torch.int32, device=dev)
    wb = int(L.bmh_cigar_pack_work(n))
    work = torch.empty(wb, dtype=torch.uint8, device=dev)
    words = L.bmh_cigar_pack_sizes(aln_t.data_ptr(), n, 1 if md_t is not None else 0, off.data_ptr(), work.data_ptr(), wb, stream)
    if words < 0:
        raise RuntimeError(f"bmh_cigar_pack_sizes rc={words}: " + _err(L))
    packed = torch.empty(max(int(words), 1), dtype=torch.int32, device=dev)
    rc = L.bmh_cigar_pack(aln_t.data_ptr(), cigar_t.data_ptr(), int(cigar_t.shape[1]), md_t.data_ptr() if md_t is not None else None,
                          int(md_t.shape[1]) if md_t is not None else 0, n, off.data_ptr(), packed.data_ptr(), stream)
    if rc != 0:
        raise RuntimeError(f"bmh_cigar_pack rc={rc}: " + _err(L))
    torch.cuda.synchronize()
    return off[:n + 1], packed[:int(words)]


def sam_text_device(po: "PostOpt", names, reads_t, offs_t, lens_t, contigs, fin_t, fin_per_read_t, slot_t, aln_t, cig_off_t, packed_t, h_rec_t=None, unflag_t=None,
                    stream: int = 0, quals_t=None, comments=None, read_groups=None) -> bytes:
    """bmh_sam_text_sizes + bmh_sam_text_write on torch CUDA tensors: the SAM text of a batch written on the device.  names: list of str;
    contigs: list of (name, length); reads_t / offs_t / lens_t: the batch's ASCII reads; the rest as sam_select_device / cigar_batch / cigar_pack
    left them.  quals_t: the qualities at offs_t (QUAL); comments: list of str (written with po.copy_comment).  Returns the text as bytes."""
    import torch
    L = load_library()
    dev = fin_t.device
    n = int(fin_per_read_t.shape[0])
    enc = [x.encode() + b"\0" for x in names]
    nblob = torch.from_numpy(np.frombuffer(b"".join(enc) or b"\0", dtype=np.uint8).copy()).to(dev)
    noff = torch.from_numpy(np.concatenate([[0], np.cumsum([len(e) for e in enc])]).astype(np.int64)).to(dev)            # [n + 1]
    cenc = [c[0].encode() + b"\0" for c in contigs]
    cblob = torch.from_numpy(np.frombuffer(b"".join(cenc), dtype=np.uint8).copy()).to(dev)
    cnoff = torch.from_numpy(np.concatenate([[0], np.cumsum([len(e) for e in cenc])]).astype(np.int32)).to(dev)         # [n_contigs + 1]
    coff = torch.from_numpy(np.concatenate([[0], np.cumsum([c[1] for c in contigs])[:-1]]).astype(np.int64)).to(dev)
    d = SamDev(n, nblob.data_ptr(), noff.data_ptr(), reads_t.data_ptr(), offs_t.data_ptr(), lens_t.data_ptr(), len(contigs), cblob.data_ptr(), cnoff.data_ptr(), coff.data_ptr(),
               fin_t.data_ptr(), fin_per_read_t.data_ptr(), slot_t.data_ptr(), aln_t.data_ptr(), cig_off_t.data_ptr(), packed_t.data_ptr(),
               h_rec_t.data_ptr() if h_rec_t is not None else None, unflag_t.data_ptr() if unflag_t is not None else None)
    if quals_t is not None:
        d.d_quals = quals_t.data_ptr()
    if comments is not None:
        cm = [x.encode() + b"\0" for x in comments]
        cmblob = torch.from_numpy(np.frombuffer(b"".join(cm) or b"\0", dtype=np.uint8).copy()).to(dev)
        cmoff = torch.from_numpy(np.concatenate([[0], np.cumsum([len(e) for e in cm])]).astype(np.int64)).to(dev)
        d.d_comments, d.d_comment_off = cmblob.data_ptr(), cmoff.data_ptr()
    if read_groups is not None:                             # (ids, group index per read): a read group per read (po.rg_id must be unset)
        gb, go = _rg_id_table(read_groups[0])
        gb_t, go_t = torch.from_numpy(gb).to(dev), torch.from_numpy(go.astype(np.int32)).to(dev)
        gr_t = torch.from_numpy(np.ascontiguousarray(read_groups[1], dtype=np.uint32).astype(np.int32)).to(dev)
        d.d_read_group, d.d_rg_ids, d.d_rg_id_off, d.n_rg = gr_t.data_ptr(), gb_t.data_ptr(), go_t.data_ptr(), len(read_groups[0])
    wb = int(L.bmh_sam_text_work(n))
    work = torch.empty(wb, dtype=torch.uint8, device=dev)
    toff = torch.empty(n + 2, dtype=torch.int64, device=dev)
    total = L.bmh_sam_text_sizes(C.byref(po), C.byref(d), toff.data_ptr(), work.data_ptr(), wb, stream)
    if total < 0:
        raise RuntimeError(f"bmh_sam_text_sizes rc={total}: " + _err(L))
    text = torch.empty(max(int(total), 1), dtype=torch.uint8, device=dev)
    rc = L.bmh_sam_text_write(C.byref(po), C.byref(d), toff.data_ptr(), text.data_ptr(), work.data_ptr(), wb, stream)
    if rc == 0:
        rc = L.bmh_sam_text_check(work.data_ptr(), n, stream)
    if rc != 0:
        raise RuntimeError(f"bmh_sam_text_write rc={rc}: " + _err(L))
    return text[: int(total)].cpu().numpy().tobytes()


class CapacityError(RuntimeError):
    """a BMH_ECAPACITY return: the device form of a stage met a read beyond its fixed limits; the caller may take the host form"""


def finalize_regs_device(index: "Index", copt, ep, po, reads_t, offs_t, regs_t, n_regs: int, regs_per_read_ptr: int, frac_rep_ptr: int, n_reads: int,
                         contigs=None, out_t=None, opr_t=None, stream: int = 0):
    """bmh_finalize_regs_device on torch CUDA tensors / device pointers (regs_per_read_ptr, frac_rep_ptr: bmh_dev_jobs_t.d_regs_per_read /
    d_frac_rep).  Returns (out int32 [m, 16] view, out_per_read int32 [n_reads]) on the device."""
    import torch
    L = load_library()
    dev = regs_t.device
    if out_t is None:
        out_t = torch.empty(max(n_regs, 1), 16, dtype=torch.int32, device=dev)
    if opr_t is None:
        opr_t = torch.empty(max(n_reads, 1), dtype=torch.int32, device=dev)
    off = np.ascontiguousarray(np.concatenate([[0], np.cumsum([c[1] for c in contigs])[:-1]]), dtype=np.int64) if contigs and len(contigs) > 1 else None
    m = L.bmh_finalize_regs_device(index.handle, C.byref(copt), C.byref(ep), C.byref(po), reads_t.data_ptr(), offs_t.data_ptr(), n_reads,
                                   regs_t.data_ptr(), n_regs, regs_per_read_ptr, frac_rep_ptr, len(contigs) if off is not None else 1,
                                   off.ctypes.data_as(C.c_void_p) if off is not None else None, out_t.data_ptr(), opr_t.data_ptr(), stream)
    if m == -3:
        raise CapacityError(f"bmh_finalize_regs_device rc={m}: " + _err(L))
    if m < 0:
        raise RuntimeError(f"bmh_finalize_regs_device rc={m}: " + _err(L))
    return out_t[:m], opr_t


def finalize_pairs(copt, ep, po, genome_len: int, pac: np.ndarray, reads_flat: np.ndarray, read_offs: np.ndarray, read_lens: np.ndarray,
                   regs: np.ndarray, regs_per_read: np.ndarray, frac_rep: np.ndarray, contigs=None, n_threads: int = 1, pe=None, out=None, device=None):
    """bmh_finalize_pairs -> (fin [m,16], per_read, h_rec, unflag, pes [4,5]).  out: optional preallocated int32 [cap,16] buffer
    (a caller that runs batch after batch keeps one, so the pages are not faulted in on every call).
    device = (Index, reads_t ASCII, offs_t, stream): bmh_finalize_pairs_dev -- the mate rescue's local alignments as one batch on the device"""
    L = load_library()
    if pe is None:
        pe = PeOpt(); L.bmh_pe_opt_default(C.byref(pe))
    n = len(read_lens)
    a = lambda x, dt: np.ascontiguousarray(x, dtype=dt)
    regs = a(regs, np.int32)
    cap = len(regs) + 2 * n + 1024          # mate rescue adds a few regions per pair; BMH_ECAPACITY (-3) if this is short: retried larger
    opr = np.zeros(max(n, 1), np.uint32); h = np.zeros(max(n, 1), np.int32); uf = np.zeros(max(n, 1), np.int32)
    pes = np.zeros((4, 5), np.float64)
    ln = a([c[1] for c in contigs], np.int32) if contigs else None
    off = a(np.concatenate([[0], np.cumsum(ln)[:-1]]), np.int64) if contigs else None
    keep = [a(pac, np.uint8), a(reads_flat, np.uint8), a(read_offs, np.uint64), a(read_lens, np.uint32), a(regs_per_read, np.uint32), a(frac_rep, np.float32)]
    if out is not None and out.dtype == np.int32 and out.ndim == 2 and out.shape[1] == 16 and out.flags.c_contiguous and len(out) >= cap:
        cap = len(out)
    else:
        out = None
    for attempt in range(4):
        if out is None or len(out) < cap:
            out = np.empty((cap, 16), np.int32)
        fn, head = L.bmh_finalize_pairs, ()
        if device is not None:
            fn, head = L.bmh_finalize_pairs_dev, (device[0].handle, device[1].data_ptr(), device[2].data_ptr(), device[3] if len(device) > 3 else None)
        m = fn(*head, C.byref(copt), C.byref(ep), C.byref(po), C.byref(pe), genome_len, _np_ptr(keep[0], _u8p), n, _np_ptr(keep[1], _u8p),
                                 _np_ptr(keep[2], _u64p), _np_ptr(keep[3], _u32p), _np_ptr(regs, _i32p), _np_ptr(keep[4], _u32p),
                                 keep[5].ctypes.data_as(C.POINTER(C.c_float)), len(contigs) if contigs else 1,
                                 off.ctypes.data_as(C.c_void_p) if contigs else None, ln.ctypes.data_as(C.c_void_p) if contigs else None,
                                 _np_ptr(out, _i32p), cap, _np_ptr(opr, _u32p), _np_ptr(h, _i32p), _np_ptr(uf, _i32p), pes.ctypes.data_as(C.c_void_p), n_threads)
        if m != -3:
            break
        cap = cap * 3 + 50 * n               # at most max_matesw rescued regions per read
    if m < 0:
        raise RuntimeError("bmh_finalize_pairs: " + _err(L))
    return out[:m], opr[:n], h[:n], uf[:n], pes


def format_sam(po: "PostOpt", names, reads_flat: np.ndarray, read_offs: np.ndarray, read_lens: np.ndarray, contigs, fin: np.ndarray,
               fin_per_read: np.ndarray, slot: np.ndarray, aln: np.ndarray, cigar: np.ndarray, md: np.ndarray, h_rec=None, unflag=None,
               as_bytes: bool = False, quals=None, comments=None, read_groups=None):
    """bmh_format_sam (or bmh_format_sam_pe when h_rec / unflag are given) on numpy arrays; contigs = list of (name, length).
    names: list of str, or (blob uint8 array of NUL-terminated names, uint64 offsets).  Returns the text as bytes if
    as_bytes, as a uint8 array over the library's own buffer if as_bytes == "view", else as str.  quals: the qualities at read_offs (QUAL; None:
    '*'); comments: (blob, offsets) as names, or None -- written with po.copy_comment (bmh_format_sam_ex / bmh_format_sam_pe_ex)."""
    L = load_library()
    if isinstance(names, tuple):
        nblob, noff = np.ascontiguousarray(names[0], dtype=np.uint8), np.ascontiguousarray(names[1], dtype=np.uint64)
    else:
        enc = [n.encode() + b"\0" for n in names]
        nblob = np.frombuffer(b"".join(enc), dtype=np.uint8)
        noff = np.concatenate([[0], np.cumsum([len(e) for e in enc])[:-1]]).astype(np.uint64) if enc else np.zeros(1, np.uint64)
    n_names = len(noff) if len(noff) else 0
    cn = (C.c_char_p * len(contigs))(*[c[0].encode() for c in contigs])
    off = np.ascontiguousarray(np.concatenate([[0], np.cumsum([c[1] for c in contigs])[:-1]]), dtype=np.int64)
    a = lambda x, dt: np.ascontiguousarray(x, dtype=dt)
    keep = [a(reads_flat, np.uint8), a(read_offs, np.uint64), a(read_lens, np.uint32), a(fin, np.int32), a(fin_per_read, np.uint32), a(slot, np.int64),
            a(aln, np.int32), a(cigar, np.uint32), a(md, np.uint8)]
    ln = C.c_size_t()
    if read_groups is not None:                             # (ids, group index per read): bmh_format_sam_groups -- a read group per read (po.rg_id must be unset)
        vp = lambda x: x.ctypes.data_as(C.c_void_p) if x is not None else None
        qq = a(quals, np.uint8) if quals is not None else None
        cb, co = (a(comments[0], np.uint8), a(comments[1], np.uint64)) if comments is not None else (None, None)
        hh, uu = (a(h_rec, np.int32), a(unflag, np.int32)) if h_rec is not None else (None, None)
        gb, go = _rg_id_table(read_groups[0])
        gr = a(read_groups[1], np.uint32)
        G = ReadGroupsT(gr.ctypes.data, gb.ctypes.data, go.ctypes.data, len(read_groups[0]))
        p = L.bmh_format_sam_groups(C.byref(po), len(read_lens), vp(nblob), _np_ptr(noff, _u64p), _np_ptr(keep[0], _u8p), _np_ptr(keep[1], _u64p), _np_ptr(keep[2], _u32p),
                                    vp(qq), vp(cb), vp(co), len(contigs), cn, vp(off), _np_ptr(keep[3], _i32p), _np_ptr(keep[4], _u32p), vp(hh), vp(uu), vp(keep[5]),
                                    _np_ptr(keep[6], _i32p), _np_ptr(keep[7], _u32p), int(keep[7].shape[1]), vp(keep[8]), int(keep[8].shape[1]), C.byref(G), C.byref(ln))
    elif quals is not None or comments is not None:
        qq = a(quals, np.uint8) if quals is not None else None
        cb, co = (a(comments[0], np.uint8), a(comments[1], np.uint64)) if comments is not None else (None, None)
        ex = (qq.ctypes.data_as(C.c_void_p) if qq is not None else None, cb.ctypes.data_as(C.c_void_p) if cb is not None else None,
              co.ctypes.data_as(C.c_void_p) if co is not None else None)
        head = (C.byref(po), len(read_lens), nblob.ctypes.data_as(C.c_void_p), _np_ptr(noff, _u64p), _np_ptr(keep[0], _u8p), _np_ptr(keep[1], _u64p), _np_ptr(keep[2], _u32p)) + ex + \
               (len(contigs), cn, off.ctypes.data_as(C.c_void_p), _np_ptr(keep[3], _i32p), _np_ptr(keep[4], _u32p))
        tail = (keep[5].ctypes.data_as(C.c_void_p), _np_ptr(keep[6], _i32p), _np_ptr(keep[7], _u32p), int(keep[7].shape[1]), keep[8].ctypes.data_as(C.c_void_p),
                int(keep[8].shape[1]), C.byref(ln))
        if h_rec is not None:
            hh, uu = a(h_rec, np.int32), a(unflag, np.int32)
            p = L.bmh_format_sam_pe_ex(*head, _np_ptr(hh, _i32p), _np_ptr(uu, _i32p), *tail)
        else:
            p = L.bmh_format_sam_ex(*head, *tail)
    elif h_rec is not None:
        hh, uu = a(h_rec, np.int32), a(unflag, np.int32)
        p = L.bmh_format_sam_pe(C.byref(po), len(read_lens), nblob.ctypes.data_as(C.c_void_p), _np_ptr(noff, _u64p), _np_ptr(keep[0], _u8p), _np_ptr(keep[1], _u64p), _np_ptr(keep[2], _u32p), len(contigs), cn,
                                off.ctypes.data_as(C.c_void_p), _np_ptr(keep[3], _i32p), _np_ptr(keep[4], _u32p), _np_ptr(hh, _i32p), _np_ptr(uu, _i32p),
                                keep[5].ctypes.data_as(C.c_void_p), _np_ptr(keep[6], _i32p), _np_ptr(keep[7], _u32p), int(keep[7].shape[1]),
                                keep[8].ctypes.data_as(C.c_void_p), int(keep[8].shape[1]), C.byref(ln))
    else:
        p = L.bmh_format_sam(C.byref(po), len(read_lens), nblob.ctypes.data_as(C.c_void_p), _np_ptr(noff, _u64p), _np_ptr(keep[0], _u8p), _np_ptr(keep[1], _u64p), _np_ptr(keep[2], _u32p), len(contigs), cn,
                             off.ctypes.data_as(C.c_void_p), _np_ptr(keep[3], _i32p), _np_ptr(keep[4], _u32p), keep[5].ctypes.data_as(C.c_void_p),
                             _np_ptr(keep[6], _i32p), _np_ptr(keep[7], _u32p), int(keep[7].shape[1]), keep[8].ctypes.data_as(C.c_void_p), int(keep[8].shape[1]),
                             C.byref(ln))
    if not p:
        raise RuntimeError("bmh_format_sam: " + _err(L))
    if as_bytes == "view":                  # the library's buffer itself as a uint8 array (freed with the array): no copy of the text
        import weakref
        arr = np.ctypeslib.as_array(C.cast(p, C.POINTER(C.c_uint8)), shape=(max(int(ln.value), 1),))[: int(ln.value)]
        weakref.finalize(arr.base if arr.base is not None else arr, L.bmh_free, C.c_void_p(p))
        return arr
    raw = C.string_at(p, ln.value)
    L.bmh_free(p)
    return raw if as_bytes else raw.decode()


def dev_jobs_to_host(j: DevJobsT, n_reads: int) -> dict:
    """Copy a bmh_dev_jobs_t to numpy arrays (test helper)."""
    import torch

    def rd(ptr, n, dt, tdt):
        if n == 0 or not ptr:
            return np.zeros(0, dt)
        buf = torch.empty(n, dtype=tdt, device="cuda")
        _memcpy_d2d(buf.data_ptr(), ptr, n * buf.element_size())
        return buf.cpu().numpy().view(dt)
    nj = int(j.n_jobs)
    out = {k: rd(getattr(j, "d_" + k), nj, np.uint32, torch.int32) for k in ("qoff", "qlen", "toff", "tlen", "h0", "job_read", "job_reg", "job_side")}
    out["q"] = rd(j.d_q, int(j.q_bytes), np.uint8, torch.uint8)
    out["t"] = rd(j.d_t, int(j.t_bytes), np.uint8, torch.uint8)
    out["regs_per_read"] = rd(j.d_regs_per_read, n_reads, np.uint32, torch.int32)
    out["frac_rep"] = rd(j.d_frac_rep, n_reads, np.float32, torch.float32)
    return out


def seeds_to_host(s: SeedsT, n_reads: int) -> dict:
    """Copy a bmh_seeds_t to numpy arrays (test/bench helper; uses torch only to read HBM).  A sampled batch is completed first (bmh_seeds_locate_all)."""
    import torch
    L = load_library()
    if L.bmh_seeds_locate_all(C.byref(s), None) != 0:
        raise RuntimeError("bmh_seeds_locate_all: " + _err(L))

    def rd(ptr, n, dt, tdt):
        if n == 0:
            return np.zeros(0, dt)
        buf = torch.empty(n, dtype=tdt, device="cuda")
        _memcpy_d2d(buf.data_ptr(), ptr, n * buf.element_size())
        return buf.cpu().numpy().view(dt)
    ns = int(s.n_seeds)
    return dict(rbeg=rd(s.d_rbeg, ns, np.uint64, torch.int64), qbeg=rd(s.d_qbeg, 2 * ns, np.int32, torch.int32).reshape(-1, 2),
                score=rd(s.d_score, ns, np.uint32, torch.int32), n_ref_pos=rd(s.d_n_ref_pos, n_reads, np.uint32, torch.int32),
                prefix=rd(s.d_prefix, n_reads, np.uint32, torch.int32))


def _memcpy_d2d(dst: int, src: int, nbytes: int) -> None:
    hip = C.CDLL("libamdhip64.so")
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    rc = hip.hipMemcpy(dst, src, nbytes, 3)  # hipMemcpyDeviceToDevice
    if rc != 0:
        raise RuntimeError(f"hipMemcpy d2d failed rc={rc}")


EXT_LONG_MAX = 16384     # BMH_EXT_LONG_MAX: the longest query bmh_extend_batch_long takes


def extend_batch(q_t, qoff_t, qlen_t, t_t, toff_t, tlen_t, h0_t, out_t, params: ExtParams | None = None, raw_t=None,
                 stream: int = 0, long_queries: bool = False, max_qlen: int = 0) -> None:
    """All arguments torch CUDA tensors; out_t int32 [n,3]; raw_t int32 [n,6] or None.  Asynchronous.
    long_queries: bmh_extend_batch_long -- queries of 769 .. max_qlen (0: EXT_LONG_MAX) bases run on the long-query kernel
    instead of coming back as INT32_MIN (bmh_extend_last_unsupported counts those beyond the cap either way)."""
    L = load_library()
    p = params or ExtParams.default()
    if long_queries:
        rc = L.bmh_extend_batch_long(q_t.data_ptr(), qoff_t.data_ptr(), qlen_t.data_ptr(), t_t.data_ptr(), toff_t.data_ptr(),
                                     tlen_t.data_ptr(), h0_t.data_ptr(), qlen_t.numel(), C.byref(p), max_qlen, out_t.data_ptr(),
                                     raw_t.data_ptr() if raw_t is not None else None, stream)
        if rc != 0:
            raise RuntimeError(f"bmh_extend_batch_long rc={rc}: " + _err(L))
        return
    rc = L.bmh_extend_batch(q_t.data_ptr(), qoff_t.data_ptr(), qlen_t.data_ptr(), t_t.data_ptr(), toff_t.data_ptr(),
                            tlen_t.data_ptr(), h0_t.data_ptr(), qlen_t.numel(), C.byref(p), out_t.data_ptr(),
                            raw_t.data_ptr() if raw_t is not None else None, stream)
    if rc != 0:
        raise RuntimeError(f"bmh_extend_batch rc={rc}: " + _err(L))


def seed_file(index_prefix: str, read_file: str, min_seed_len: int = 19) -> dict:
    """The reference's call sequence (src/fastmap.c:436-465) through the drop-in C ABI:
    bwt_restore_bwt_gpu -> bwt_restore_sa_gpu -> gpu_cpy_wrapper -> seed_gpu -> free_gpuseed_data."""
    L = load_library()
    libc = C.CDLL(None)
    libc.free.argtypes = [C.c_void_p]
    d = GpuseedStorageVector()
    d.query_file = index_prefix.encode()
    d.read_file = read_file.encode()
    d.file_bytes_skip = 0
    d.min_seed_size = min_seed_len
    d.is_smem = 1
    d.bwt = L.bwt_restore_bwt_gpu((index_prefix + ".bwt").encode())
    L.bwt_restore_sa_gpu((index_prefix + ".sa").encode(), d.bwt)
    d.bwt_gpu = L.gpu_cpy_wrapper(d.bwt)
    d.pre_calc_seed_len = 13
    d.pre_calc_seed_intervals_flag = 0
    res = L.seed_gpu(C.byref(d))
    n_reads = int(L.seed_gpu_last_n_reads())
    L.free_gpuseed_data(C.byref(d))
    r = res.contents
    n_ref = np.ctypeslib.as_array(r.n_ref_pos_fow_rev_results, shape=(max(n_reads, 1),))[:n_reads].copy()
    prefix = np.ctypeslib.as_array(r.n_ref_pos_fow_rev_prefix_sums, shape=(max(n_reads, 1),))[:n_reads].copy()
    ns = int(n_ref.sum())
    out = dict(rbeg=np.ctypeslib.as_array(r.rbeg, shape=(max(ns, 1),))[:ns].copy(),
               qbeg=np.ctypeslib.as_array(r.qbeg, shape=(max(2 * ns, 1),))[:2 * ns].copy().reshape(-1, 2),
               score=np.ctypeslib.as_array(r.score, shape=(max(ns, 1),))[:ns].copy(),
               n_ref_pos=n_ref, prefix=prefix, file_bytes=int(r.file_bytes_skip))
    for p in (r.rbeg, r.qbeg, r.score, r.n_ref_pos_fow_rev_results, r.n_ref_pos_fow_rev_prefix_sums):
        libc.free(C.cast(p, C.c_void_p))
    libc.free(C.cast(res, C.c_void_p))
    return out


class HostJobs:
    """Host job builder (bmh_build_jobs): chains -> filtered chains -> extension jobs, per read."""

    def __init__(self, genome_fwd: np.ndarray, reads: np.ndarray, read_offs: np.ndarray, read_lens: np.ndarray, seeds: dict,
                 n_threads: int = 0, opt: "ChainOpt | None" = None, contigs=None, pac: "np.ndarray | None" = None):
        """contigs: optional list of (name, length) -- the sequences of the packed reference, in order; pac: the 2-bit forward strand
        if the caller has it already (packing a 3.1 Gbp genome takes seconds; self.t_pack tells how long it took here)"""
        import time as _time
        L = load_library()
        self.L = L
        o = opt or ChainOpt()
        if opt is None:
            L.bmh_chain_opt_default(C.byref(o))
        self.opt = o
        self._genome = genome_fwd
        l_pac = int(genome_fwd) if np.isscalar(genome_fwd) else int(genome_fwd.shape[0])       # (a length, when the caller passes the pac)
        self.l_pac = l_pac
        _t0 = _time.time()
        if pac is None:
            pad = (-l_pac) % 4
            codes = np.concatenate([genome_fwd, np.zeros(pad, np.uint8)]).reshape(-1, 4)
            pac = np.ascontiguousarray(((codes[:, 0] << 6) | (codes[:, 1] << 4) | (codes[:, 2] << 2) | codes[:, 3]).astype(np.uint8))
        else:
            pac = np.ascontiguousarray(pac, dtype=np.uint8)
        self.t_pack = _time.time() - _t0
        a = lambda x, dt: np.ascontiguousarray(x, dtype=dt)
        self._keep = [pac, a(reads, np.uint8), a(read_offs, np.uint64), a(read_lens, np.uint32), a(seeds["rbeg"], np.uint64),
                      a(seeds["qbeg"], np.int32), a(seeds["score"], np.uint32), a(seeds["n_ref_pos"], np.uint32), a(seeds["prefix"], np.uint32)]
        k = self._keep
        self.n_contigs = len(contigs) if contigs else 1
        self.ctg_len = np.ascontiguousarray([c[1] for c in contigs], dtype=np.int32) if contigs else None
        self.ctg_off = np.ascontiguousarray(np.concatenate([[0], np.cumsum(self.ctg_len)[:-1]]), dtype=np.int64) if contigs else None
        self.h = L.bmh_build_jobs(C.byref(o), l_pac, _np_ptr(k[0], _u8p), self.n_contigs,
                                  self.ctg_off.ctypes.data_as(C.c_void_p) if contigs else None, self.ctg_len.ctypes.data_as(C.c_void_p) if contigs else None,
                                  len(k[3]), _np_ptr(k[1], _u8p),
                                  _np_ptr(k[2], _u64p), _np_ptr(k[3], _u32p), _np_ptr(k[4], _u64p), _np_ptr(k[5], _i32p),
                                  _np_ptr(k[6], _u32p), _np_ptr(k[7], _u32p), _np_ptr(k[8], _u32p), n_threads or (os.cpu_count() or 1))
        if not self.h:
            raise RuntimeError("bmh_build_jobs: " + _err(L))
        sz = [C.c_uint64() for _ in range(4)]
        L.bmh_jobs_sizes(self.h, *[C.byref(x) for x in sz])
        self.n_jobs, self.n_regs, qb, tb = (int(x.value) for x in sz)
        ptrs = [C.c_void_p() for _ in range(11)]
        L.bmh_jobs_arrays(self.h, *[C.byref(p) for p in ptrs])

        def view(p, n, dt):
            if n == 0:
                return np.zeros(0, dt)
            return np.ctypeslib.as_array(C.cast(p, C.POINTER(C.c_uint8 if dt == np.uint8 else C.c_uint32)), shape=(n,)).view(dt)
        nj = self.n_jobs
        self.q = view(ptrs[0], qb, np.uint8); self.qoff = view(ptrs[1], nj, np.uint32); self.qlen = view(ptrs[2], nj, np.uint32)
        self.t = view(ptrs[3], tb, np.uint8); self.toff = view(ptrs[4], nj, np.uint32); self.tlen = view(ptrs[5], nj, np.uint32)
        self.h0 = view(ptrs[6], nj, np.uint32); self.job_read = view(ptrs[7], nj, np.uint32); self.job_reg = view(ptrs[8], nj, np.uint32)
        self.job_side = view(ptrs[9], nj, np.uint32); self.regs_per_read = view(ptrs[10], len(k[3]), np.uint32)

    def jobs(self):
        q = self.q if self.q.size else np.zeros(1, np.uint8)
        t = self.t if self.t.size else np.zeros(1, np.uint8)
        return q, self.qoff, self.qlen, t, self.toff, self.tlen, self.h0

    def merge(self, out3: np.ndarray) -> np.ndarray:
        out3 = np.ascontiguousarray(out3, dtype=np.int32)
        regs = np.zeros((max(self.n_regs, 1), 8), np.int32)
        self.L.bmh_merge_regs(self.h, _np_ptr(out3, _i32p), _np_ptr(regs, _i32p))
        return regs[: self.n_regs]

    def frac_rep(self) -> np.ndarray:
        n = len(self._keep[3])
        return np.ctypeslib.as_array(self.L.bmh_jobs_frac_rep(self.h), shape=(max(n, 1),))[:n].copy()

    def finalize(self, regs: np.ndarray, flag_all: bool = False, id0: int = 0, params: "ExtParams | None" = None, n_threads: int = 1):
        """bmh_finalize_regs on the regions of merge(): -> (out int32 [m, 16], out_per_read uint32 [n_reads])"""
        L = self.L
        po = PostOpt(); L.bmh_post_opt_default(C.byref(po)); po.flag_all = 1 if flag_all else 0; po.id0 = id0
        co = self.opt
        ep = params or ExtParams.default()
        k = self._keep
        regs = np.ascontiguousarray(regs, dtype=np.int32)
        out = np.zeros((max(len(regs), 1), 16), np.int32); opr = np.zeros(max(len(k[3]), 1), np.uint32)
        fr = np.ascontiguousarray(self.frac_rep(), dtype=np.float32)
        m = L.bmh_finalize_regs(C.byref(co), C.byref(ep), C.byref(po), self.l_pac, _np_ptr(k[0], _u8p), len(k[3]), _np_ptr(k[1], _u8p),
                                _np_ptr(k[2], _u64p), _np_ptr(regs, _i32p), _np_ptr(np.ascontiguousarray(self.regs_per_read), _u32p),
                                fr.ctypes.data_as(C.POINTER(C.c_float)), self.n_contigs,
                                self.ctg_off.ctypes.data_as(C.c_void_p) if self.ctg_off is not None else None,
                                _np_ptr(out, _i32p), _np_ptr(opr, _u32p), n_threads)
        if m < 0:
            raise RuntimeError("bmh_finalize_regs: " + _err(L))
        return out[:m], opr[: len(k[3])]

    def free(self):
        if self.h:
            self.L.bmh_jobs_free(self.h)
            self.h = None
