"""bwamem_hip -- host-side Python mirror of the MI355X seed-and-extend library.

The product is libbwamem_hip.so (hand-written HIP for gfx950, C ABI declared in
include/bwamem_hip.h and include/seed_gen.h).  This package only binds it with
ctypes for tests, bench.py and the multi-GPU launcher, and carries the
synthetic-data and index-building tooling.  There is no CPU implementation of
the hot path in here: if the shared library or a HIP device is missing, calls
raise.
"""
from . import fmindex, synth  # noqa: F401
from .index import fasta_pack, index_fasta  # noqa: F401
from .lib import (ExtParams, HipLibraryMissing, Index, SeedWorkspace, extend_batch, lib_path,  # noqa: F401
                  bam_stats, load_library, seed_file)
from .lib import bam_apply_recal, bam_recal, known_sites_mask, recal_apply_tables  # noqa: F401
from .recal import read_recal_table, recal_apply_report_text, recal_empirical_quality, recal_table_text  # noqa: F401


def insert_size_metrics(hist, smallest, largest) -> dict:
    """bwamem_hip.aligner.insert_size_metrics: median, MAD, mode, trimmed mean and SD of one orientation's insert-size histogram"""
    from .aligner import insert_size_metrics as f
    return f(hist, smallest, largest)


def bam_post_file(*args, **kw):
    """bwamem_hip.bam.bam_post_file (imported on first use, so that `python -m bwamem_hip.bam` finds its module unloaded)"""
    from .bam import bam_post_file as f
    return f(*args, **kw)
