"""The options of duplicate marking as one record, on the device: over test_markdup_options' stream and combinations the device calls give the records, the file,
the index and the counts of the host calls -- bam_markdup under every combination, bam_sorted_file under every one without an optical distance, with a BAI and
with a CSI index.  All comparisons are exact."""
import pytest

from bwamem_hip.lib import bam_markdup, bam_sorted_file
from test_bam_dup import CONTIGS
from test_markdup_options import COMBOS, HDR, host_markdup, kw_id, stream

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("kw", COMBOS, ids=kw_id)
def test_markdup_device_equals_host(kw):
    assert bam_markdup(stream(), host=False, **kw) == host_markdup(kw)


@pytest.mark.parametrize("index_format", ("bai", "csi"))
@pytest.mark.parametrize("kw", [k for k in COMBOS if "optical_distance" not in k], ids=kw_id)
def test_sorted_file_device_equals_host(kw, index_format):
    ix = dict(index_format=index_format, csi_min_shift=12) if index_format == "csi" else {}
    want = bam_sorted_file(HDR, CONTIGS, stream(), host=True, markdup=True, window=25, **ix, **kw)
    assert bam_sorted_file(HDR, CONTIGS, stream(), host=False, markdup=True, window=25, **ix, **kw) == want
    assert want[2] == host_markdup(kw)[1]
