"""A run from a read file that fails part-way -- the write callback raises on its second call -- and the same aligner used again: the run raises that exception,
nothing hangs (the loader's queue, the lanes and the writer all end), and the next run of the same object writes what a fresh aligner writes.  align_file and
align_files (the two loaders of csrc/align_pipeline.hip over csrc/batch_queue.h), SAM and BAM (the output stage)."""
import faulthandler

import pytest

from test_bam_gpu import PREFIX, _reads_files, hip  # noqa: F401 -- hip: the fixture


class _Refused(Exception):
    pass


class _Out:
    """a binary file object; fail_at k: the aligner's k-th call of its write callback raises (a batch arrives as a memoryview, the headers and the end-of-file member as bytes)"""
    mode = "wb"

    def __init__(self, fail_at=0):
        self.data, self.calls, self.fail_at, self.raised = bytearray(), 0, fail_at, None

    def write(self, b):
        if isinstance(b, memoryview):
            self.calls += 1
            if self.calls == self.fail_at:
                self.raised = _Refused("call %d of the write callback" % self.calls)
                raise self.raised
        self.data += b


@pytest.mark.gpu
@pytest.mark.parametrize("fmt", ["sam", "bam"])
@pytest.mark.parametrize("entry", ["align_file", "align_files"])
def test_failed_run_then_the_same_aligner_again(hip, tmp_path, entry, fmt):
    from bwamem_hip.aligner import Aligner
    path = _reads_files(tmp_path, False, n=2000, L=100)                    # 200 000 bases: five batches of 40 000

    def run(al, out):
        kw = dict(chunk_bases=40_000, fmt=fmt)
        return al.align_file(path, out, **kw) if entry == "align_file" else al.align_files(path, out=out, **kw)
    faulthandler.dump_traceback_later(120, exit=True)                     # a plain time limit: a run that hangs ends the process
    try:
        al = Aligner(PREFIX, n_threads=4)
        bad = _Out(fail_at=2)
        with pytest.raises(_Refused) as ei:
            run(al, bad)
        assert ei.value is bad.raised and bad.calls == 2
        again = _Out()
        assert run(al, again) == 2000 and again.calls >= 4
        fresh_al = Aligner(PREFIX, n_threads=4)
        fresh = _Out()
        assert run(fresh_al, fresh) == 2000
        assert bytes(again.data) == bytes(fresh.data) and len(fresh.data) > 200_000 // (4 if fmt == "bam" else 1)
        al.close(); fresh_al.close()
    finally:
        faulthandler.cancel_dump_traceback_later()
