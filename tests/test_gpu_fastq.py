"""GPU: SeqSet.from_fastq (pg_fastq.hip: k_fastq_scan, k_fastq_offsets, k_fastq_join, then k_pack) on the crafted texts of
tests/place_ref.py — the unpacked contig, nreads and consumed exactly the model's (Python's split), malformed records refused, and
the joined reads counting like the model's joined sequence loaded from the host."""
import ctypes as C

import numpy as np
import pytest

from tests import place_ref as pr

pytestmark = pytest.mark.gpu

PG_E_INVALID = -1
TEXTS = pr.fastq_texts()


def _check(ctx, text, tag):
    from panagram_amd import engine
    joined, nreads, consumed = pr.fastq_model(text)
    ss, n, used = engine.SeqSet.from_fastq(ctx, text)
    try:
        assert (n, used) == (nreads, consumed), tag
        assert ss.names == [""] and ss.lens.tolist() == [len(joined)], tag
        got = ss.unpack(0)
        want = pr.as_packed(joined)
        if got != want:
            at = next(i for i, (a, b) in enumerate(zip(got, want)) if a != b)
            raise AssertionError(f"{tag}: base {at} of {len(want)}: {got[at - 5:at + 5]!r} != {want[at - 5:at + 5]!r}")
        return got
    finally:
        ss.close()


@pytest.mark.parametrize("name", sorted(TEXTS))
def test_from_fastq_equals_the_model(ctx, name):
    _check(ctx, TEXTS[name], name)


def test_from_fastq_of_a_uint8_array_and_of_every_cut_of_a_small_text(ctx):
    """every prefix of three records (each of the four lines cut at every byte), as bytes and as a uint8 array"""
    text = pr.fastq_text([b"ACGTAC", b"", b"GGt"], eol=b"\r\n")
    for cut in range(len(text) + 1):
        _check(ctx, text[:cut], f"cut at {cut}")
    _check(ctx, np.frombuffer(text, np.uint8), "array")


def test_no_complete_record_is_one_contig_of_length_zero(ctx):
    """consumed == 0: pg_seqset_create allows a contig without a base, so the seqset has one"""
    from panagram_amd import engine
    for text in (b"", b"@r0\nACGT\n+\n", b"\n"):
        ss, n, used = engine.SeqSet.from_fastq(ctx, text)
        try:
            assert (n, used) == (0, 0) and ss.lens.tolist() == [0] and ss.unpack(0) == b"" and ss.total_kmers(21) == 0
        finally:
            ss.close()


@pytest.mark.parametrize("name", sorted(pr.fastq_malformed_texts()))
def test_malformed_records_are_refused(ctx, name):
    from panagram_amd import engine
    text, bad = pr.fastq_malformed_texts()[name]
    with pytest.raises(engine.PanagramHipError) as ei:
        engine.SeqSet.from_fastq(ctx, text)
    assert ei.value.code == PG_E_INVALID
    msg = str(ei.value)
    rec = int(msg.split("record ")[1].split(":")[0])
    assert rec in bad, (msg, bad[:5])
    assert ("'@'" in msg) == (name != "no_plus"), msg
    # no seqset: the handle stays NULL
    h, n, used = C.c_void_p(), C.c_uint64(7), C.c_uint64(7)
    buf = np.frombuffer(text, np.uint8)
    code = ctx._lib.pg_seqset_from_fastq(ctx._h, buf.ctypes.data_as(C.c_void_p), len(buf), C.byref(h), C.byref(n), C.byref(used))
    assert code == PG_E_INVALID and not h.value
    # a malformed record behind the last complete one is not looked at
    good = pr.fastq_text([b"ACGT", b"GGCC"])
    _check(ctx, good + b"xr\nAC\n-\n", "torn and malformed")


def test_null_arguments(ctx):
    h, n = C.c_void_p(), C.c_uint64()
    lib = ctx._lib
    assert lib.pg_seqset_from_fastq(ctx._h, None, 5, C.byref(h), C.byref(n), C.byref(n)) == PG_E_INVALID
    assert lib.pg_seqset_from_fastq(ctx._h, None, 0, None, C.byref(n), C.byref(n)) == PG_E_INVALID
    assert lib.pg_seqset_from_fastq(None, None, 0, C.byref(h), C.byref(n), C.byref(n)) == PG_E_INVALID


def test_counting_a_fastq_seqset_equals_counting_the_joined_model(ctx):
    """CopyTable.count of a from_fastq seqset == of SeqSet.from_host([the model's joined sequence]), plane by plane"""
    from panagram_amd import engine
    rng = np.random.default_rng(5)
    k = pr.FASTQ_K
    target = pr.rand(rng, 5000)
    reads = []
    for s in rng.integers(0, 5000 - 120, 400):
        r = target[int(s):int(s) + int(rng.integers(1, 120))]
        reads.append(r if rng.random() < 0.5 else pr.revcomp(r))
    reads += [b"", target[:k - 1], target[100:100 + k]] * 3
    text = pr.fastq_text(reads, eol=b"\r\n")
    tss = engine.SeqSet.from_host(ctx, [target])
    table = engine.CopyTable(ctx, k, 5000, 2)
    fq, n, used = engine.SeqSet.from_fastq(ctx, text)
    host = engine.SeqSet.from_host(ctx, [pr.fastq_model(text)[0]])
    try:
        table.insert(tss)
        assert n == len(reads) and used == len(text)
        h0, h1 = table.count(0, fq), table.count(1, host)
        hist, valid, depth = table.profile(tss, track=True)
        assert h0 == h1 > 1000 and np.array_equal(depth[0], depth[1]) and np.array_equal(hist[:, 0], hist[:, 1])
        assert depth[0].max() >= 4  # (reads of k - 1 bases add nothing, the read of k bases adds three)
    finally:
        for x in (host, fq, table, tss):
            x.close()
