"""GPU: SeqSet.from_fastq (pg_fastq.hip: k_fastq_scan, k_fastq_offsets, k_fastq_join, then k_pack) on the texts of
tests/fastq_craft.py, which tests/test_fastq_craft_cpu.py proves to hold the edges they are named for: a byte pair split between two
lanes' loads or two tiles, tiles that start in every line class on a line and mid-line, tiles behind the last complete record,
lengths that fill the last lane or tile, 255 to 513 tiles, and malformed lines at all of these.  Accepted texts equal the model
byte for byte; a refused text names the FIRST malformed line's record and kind; batches of place.FastqBatches reassemble the file."""
import ctypes as C
import gzip

import numpy as np
import pytest

from tests import fastq_craft as fc
from tests.test_gpu_fastq import PG_E_INVALID, _check

pytestmark = pytest.mark.gpu

T = fc.T
GOOD, BAD = fc.well_formed(), fc.malformed()


@pytest.mark.parametrize("name", sorted(GOOD))
def test_crafted_text_equals_the_model(ctx, name):
    """nreads, consumed, the length and every base as the split-based model has them (and so as ``walk``: the CPU test holds the
    two together); a second call gives the same bytes"""
    text = GOOD[name].text
    first = _check(ctx, text, name)
    joined, nreads, consumed, first_bad = fc.walk(text)
    assert first_bad is None and first == fc.as_packed(joined), name
    assert _check(ctx, text, name + " (again)") == first, name


@pytest.mark.parametrize("name", sorted(BAD))
def test_crafted_malformed_text_is_refused_for_its_first_malformed_line(ctx, name):
    from panagram_amd import engine
    text = BAD[name].text
    record, kind = fc.walk(text)[3]
    with pytest.raises(engine.PanagramHipError) as ei:
        engine.SeqSet.from_fastq(ctx, text)
    assert ei.value.code == PG_E_INVALID
    msg = str(ei.value)
    got = int(msg.split("record ")[1].split(":")[0])
    got_kind = {(True, False): "header", (False, True): "separator"}[("'@'" in msg, "'+'" in msg)]
    assert (got, got_kind) == (record, kind), msg
    # no seqset: the handle stays NULL
    h, n, used = C.c_void_p(), C.c_uint64(7), C.c_uint64(7)
    buf = np.frombuffer(text, np.uint8)
    code = ctx._lib.pg_seqset_from_fastq(ctx._h, buf.ctypes.data_as(C.c_void_p), len(buf), C.byref(h), C.byref(n), C.byref(used))
    assert code == PG_E_INVALID and not h.value


def _stream(ctx, path, batch_bytes):
    """(the batches' contigs joined by N, reads, batches without a complete record) of the file under from_fastq"""
    from panagram_amd import engine
    from panagram_amd import place as pl
    fb = pl.FastqBatches(path, batch_bytes)
    parts, reads, empty = [], 0, 0
    for buf in fb:
        ss, n, used = engine.SeqSet.from_fastq(ctx, buf)
        try:
            assert 0 <= used <= len(buf) and (n == 0) == (used == 0), batch_bytes
            if n:
                parts.append(ss.unpack(0))
            else:
                assert ss.lens.tolist() == [0], batch_bytes
                empty += 1
            reads += n
        finally:
            ss.close()
        fb.advance(used)
    return b"N".join(parts), reads, empty


def test_batches_of_a_crlf_file_reassemble_the_whole(ctx, tmp_path):
    """FastqBatches, ``consumed`` and the carried tail at batch sizes around a tile: a read longer than three tiles leaves batches
    without a complete record (consumed == 0), the line ends are torn between "\\r" and "\\n" """
    whole = fc.batch_text()
    joined, nreads, consumed = fc.fastq_model(whole)
    want = fc.as_packed(joined)
    plain, gz = str(tmp_path / "reads.fq"), str(tmp_path / "reads.fq.gz")
    open(plain, "wb").write(whole)
    with gzip.open(gz, "wb") as f:
        f.write(whole)
    for path, sizes in ((plain, fc.BATCH_SIZES), (gz, fc.BATCH_SIZES[:1])):
        for b in sizes:
            got, reads, empty = _stream(ctx, path, b)
            assert reads == nreads and empty >= 1, (path, b, reads, empty)
            if got != want:
                at = next((i for i, (x, y) in enumerate(zip(got, want)) if x != y), min(len(got), len(want)))
                raise AssertionError(f"batches of {b}: base {at} of {len(want)} ({len(got)} joined)")
