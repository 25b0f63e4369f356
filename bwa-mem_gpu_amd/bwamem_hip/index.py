"""`bwa index` on the device: a FASTA (or .fa.gz) reference -> prefix.{bwt,sa,pac,ann,amb} (include/bwamem_hip.h
bmh_index_fasta, csrc/fasta_pack.hip).  The files are byte for byte what the reference's two-pass `bwa index` writes and
load with Aligner(prefix).

    python -m bwamem_hip.index [-p PREFIX] [-r INT] [--verify] [--chunk-bytes N] [--device cuda:0] ref.fa[.gz]

Unlike `bwa index -r`, the SA interval must be a power of two (the device builder's sampling).
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

from .lib import _err, load_library

BMH_EINVAL = -2


class IndexFastaStats(C.Structure):
    """bmh_index_fasta_stats_t"""
    _fields_ = [("n_contigs", C.c_uint64), ("n_holes", C.c_uint64), ("l_pac", C.c_uint64), ("n_ambig", C.c_uint64), ("file_bytes", C.c_uint64),
                ("read_seconds", C.c_double), ("h2d_seconds", C.c_double), ("pack_seconds", C.c_double), ("build_seconds", C.c_double),
                ("write_seconds", C.c_double), ("total_seconds", C.c_double), ("verified", C.c_int)]


class FastaPacked(C.Structure):
    """bmh_fasta_packed_t"""
    _fields_ = [("d_pac", C.c_void_p), ("pac_bytes", C.c_uint64), ("l_pac", C.c_uint64), ("n_ambig", C.c_uint64),
                ("n_contigs", C.c_int32), ("names", C.c_void_p), ("comments", C.c_void_p), ("name_off", C.c_void_p), ("comment_off", C.c_void_p),
                ("offsets", C.c_void_p), ("lens", C.c_void_p), ("n_ambs", C.c_void_p),
                ("n_holes", C.c_int64), ("hole_off", C.c_void_p), ("hole_len", C.c_void_p), ("hole_char", C.c_void_p)]


def _lib():
    L = load_library()
    L.bmh_index_fasta.restype = C.c_int
    L.bmh_index_fasta.argtypes = [C.c_char_p, C.c_char_p, C.c_int, C.c_int, C.c_size_t, C.POINTER(IndexFastaStats)]
    L.bmh_fasta_pack.restype = C.c_int
    L.bmh_fasta_pack.argtypes = [C.c_char_p, C.c_size_t, C.POINTER(FastaPacked), C.POINTER(IndexFastaStats)]
    L.bmh_fasta_packed_free.argtypes = [C.POINTER(FastaPacked)]
    return L


def _raise(L, rc: int, what: str):
    msg = _err(L)
    if rc == BMH_EINVAL:
        raise ValueError(f"{what}: {msg}")
    raise RuntimeError(f"{what} rc={rc}: {msg}")


def _set_device(L, device) -> None:
    import torch
    dev = torch.device(device)
    idx = dev.index if dev.index is not None else 0
    torch.cuda.set_device(idx)
    if L.bmh_set_device(idx) != 0:
        raise RuntimeError("bmh_set_device: " + _err(L))


def _stats(st: IndexFastaStats) -> dict:
    return {k: getattr(st, k) for k, _ in IndexFastaStats._fields_}


def index_fasta(fasta: str, prefix: str | None = None, sa_intv: int = 16, verify: bool = False, device="cuda:0",
                chunk_bytes: int | None = None) -> dict:
    """bmh_index_fasta: writes prefix.{bwt,sa,pac,ann,amb} (prefix defaults to the FASTA's path, as in `bwa index`);
    returns the stats.  A malformed file or a non-power-of-two sa_intv raises ValueError and writes nothing."""
    L = _lib()
    _set_device(L, device)
    st = IndexFastaStats()
    rc = L.bmh_index_fasta(str(fasta).encode(), str(prefix if prefix is not None else fasta).encode(), int(sa_intv),
                           1 if verify else 0, int(chunk_bytes or 0), C.byref(st))
    if rc != 0:
        _raise(L, rc, "bmh_index_fasta")
    return _stats(st)


def fasta_pack(fasta: str, device="cuda:0", chunk_bytes: int | None = None) -> dict:
    """bmh_fasta_pack: the device .pac body (copied to a numpy uint8 array of ceil(l_pac/4) bytes) and the contig and hole
    tables of the .ann / .amb."""
    L = _lib()
    _set_device(L, device)
    pk = FastaPacked()
    st = IndexFastaStats()
    rc = L.bmh_fasta_pack(str(fasta).encode(), int(chunk_bytes or 0), C.byref(pk), C.byref(st))
    if rc != 0:
        _raise(L, rc, "bmh_fasta_pack")
    try:
        l_pac, n, nh = int(pk.l_pac), int(pk.n_contigs), int(pk.n_holes)
        pac = np.empty((l_pac + 3) // 4, np.uint8)
        if pac.size:
            _copy_d2h(pac, pk.d_pac)

        def arr(ptr, count, dt):
            if count == 0:
                return np.zeros(0, dt)
            return np.ctypeslib.as_array(C.cast(ptr, C.POINTER(np.ctypeslib.as_ctypes_type(dt))), shape=(count,)).copy()

        def strings(base, offs):
            return [C.string_at(base + int(o)).decode("latin-1") for o in offs]
        return dict(pac=pac, l_pac=l_pac, n_ambig=int(pk.n_ambig),
                    names=strings(pk.names, arr(pk.name_off, n, np.uint64)), comments=strings(pk.comments, arr(pk.comment_off, n, np.uint64)),
                    offsets=arr(pk.offsets, n, np.int64), lens=arr(pk.lens, n, np.int64), n_ambs=arr(pk.n_ambs, n, np.int32),
                    hole_off=arr(pk.hole_off, nh, np.int64), hole_len=arr(pk.hole_len, nh, np.int64),
                    hole_char=arr(pk.hole_char, nh, np.uint8), stats=_stats(st))
    finally:
        L.bmh_fasta_packed_free(C.byref(pk))


def _copy_d2h(dst: np.ndarray, d_ptr: int) -> None:
    """hipMemcpy of a device buffer the library owns, through the HIP runtime the library runs on (the one loaded in this process)"""
    path = next((ln.split()[-1] for ln in open("/proc/self/maps") if "libamdhip64.so" in os.path.basename(ln.split()[-1])), None)
    if path is None:
        raise RuntimeError("the HIP runtime is not loaded")
    hip = C.CDLL(path)
    hip.hipMemcpy.restype = C.c_int
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    rc = hip.hipMemcpy(dst.ctypes.data, d_ptr, dst.nbytes, 2)      # hipMemcpyDeviceToHost
    if rc != 0:
        raise RuntimeError(f"hipMemcpy of the packed text failed: {rc}")


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(prog="python -m bwamem_hip.index", description="bwa index on the device: FASTA (or .fa.gz) -> .bwt .sa .pac .ann .amb")
    ap.add_argument("fasta")
    ap.add_argument("-p", dest="prefix", default=None, help="prefix of the output files [same as the FASTA]")
    ap.add_argument("-r", dest="sa_intv", type=int, default=16, help="SA sampling interval, a power of two [16]")
    ap.add_argument("--verify", action="store_true", help="check the suffix array completely before writing")
    ap.add_argument("--chunk-bytes", type=int, default=None, help="bytes of the file packed per chunk [256 MiB]")
    ap.add_argument("--device", default="cuda:0")
    a = ap.parse_args(argv)
    try:
        st = index_fasta(a.fasta, a.prefix, a.sa_intv, a.verify, a.device, a.chunk_bytes)
    except ValueError as e:
        print(f"[bwamem_hip.index] {e}", file=sys.stderr)
        return 1
    print(json.dumps(st))
    return 0


if __name__ == "__main__":
    sys.exit(main())
