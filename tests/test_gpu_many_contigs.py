"""GPU: sequence sets of thousands of short contigs (tests/many_contigs.py) through every path that does work per contig,
against the references the suite already has, exactly.

What the counts reach that no smaller set does:
  k_tile0 (one block of 1024 threads, ceil(n / 1024) consecutive contigs per thread): two contigs per thread at 1025, three at
  2049 and 3000; the run of 12 empty contigs in the middle holds whole shares that sum to 0; the empty runs at the front and
  at the end are the equal entries k_insert_tile's search in tile0 has to step over.
  pg_table's tile0 array (room for max(1024, 2 (n + 1)) words, regrown behind a stream synchronisation): sets of 10, 1024 and
  2051 contigs into one table need 11, 1025 (> 1024) and 2052 (> 2050) words — both regrowths.
  The epilogues' look-aheads in tile_contig, k_lowres, contigs_small, contig_colsums, run_range, coschedule and write_bgzf:
  nearly every contig is one tile or less, so every look-ahead crosses a contig.
  SeqSet.from_fasta: k_text_scan's one block per record, several records per 4096-byte window, and 65535 / 65536 / 65537 header
  lines in a text of more than 4 MB — at the cap of the device's header list, and past it, where the host scans for itself."""
import functools
import gzip

import numpy as np
import pytest

from oracle import pyoracle as po
from panagram_amd import search
from tests import blocks_ref as br
from tests import many_contigs as mc
from tests import minhash_ref
from tests import search_ref
from tests import synteny_ref as sr
from tests import variants_ref as vr
from tests.test_gpu_probe_spans import _oracle_contig

pytestmark = pytest.mark.gpu

K = 21
SEED = 7
KPL = 1.25                                   # keys per line the byte-mask tables are created for
SPAN = {40: 40_000, 70: 12_000, 100: 12_000, 130: 6_000}  # bases of the genomes behind g0 in the wide tables
SLOTS = {3: 8, 8: 14, 70: 6, 100: 16}        # keys per table line: 8-slot, byte-mask, inline and split lines


def _tile():
    from panagram_amd import engine
    return engine.tile_positions()


@functools.lru_cache(maxsize=None)
def case(ngenomes, k, n, ends_empty=True):
    """(genomes, the oracle's databases): g0 cut into n contigs, the others diverged copies — whole up to 8 genomes, windows
    of SPAN bases spread over the sequence in the wide tables.  Computed once, left alone."""
    genomes = mc.genomes(ngenomes, k, n, SEED, _tile(), span=SPAN.get(ngenomes, 0), ends_empty=ends_empty)
    return genomes, po.build_bitvec_dbs(genomes, k)


@functools.lru_cache(maxsize=None)
def contig_oracle(ngenomes, k, n):
    """per contig of g0: None without a k-mer, else (rows, rows100, bins, column sums) — po.anchor_contig; for a contig of
    fewer than 100 k-mers the project's rule of one bin per k-mer (tests/test_gpu_probe_spans.py: _oracle_contig)"""
    genomes, dbs = case(ngenomes, k, n)
    return [_oracle_contig(dbs, seq, k, ngenomes) if len(seq) >= k else None for seq in genomes[0]]


def _nkeys(dbs):
    return len(np.unique(np.concatenate([d[0] for d in dbs])))


def _new_table(ctx, k, ngenomes, nkeys):
    from panagram_amd import engine
    if ngenomes == 8:
        return engine.PanTable(ctx, k, ngenomes, expected_keys=int(nkeys * 1.02) + 64, keys_per_line=KPL)
    return engine.PanTable(ctx, k, ngenomes)


def _build(ctx, genomes, k, nkeys):
    from panagram_amd import engine
    tbl = _new_table(ctx, k, len(genomes), nkeys)
    for g, contigs in enumerate(genomes):
        ss = engine.SeqSet.from_host(ctx, contigs)
        tbl.insert_seqset(g, ss)
        ss.close()
    return tbl


def _export_equals(tbl, dbs, tag=""):
    for d, (fk, fm) in enumerate(dbs):
        keys, vals = tbl.export(d)
        o = np.argsort(keys, kind="stable")
        assert len(keys) == len(fk), (tag, d, len(keys), len(fk))
        assert np.array_equal(keys[o], fk) and np.array_equal(vals[o], fm), (tag, d)


# ---------------------------------------------------------------------------
# build
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("ngenomes", sorted(SLOTS))
@pytest.mark.parametrize("n", mc.COUNTS)
def test_build_of_a_fragmented_genome_equals_the_oracle(ctx, n, ngenomes):
    """insert_seqset of every genome, g0 in n contigs (k_tile0 with 2 and 3 contigs per thread and shares that sum to 0;
    k_insert_tile's search over the runs of equal entries), once per table layout: the exported sets and the key count are the
    oracle's"""
    genomes, dbs = case(ngenomes, K, n)
    nkeys = _nkeys(dbs)
    tbl = _build(ctx, genomes, K, nkeys)
    try:
        st = tbl.stats()
        assert st["nslots"] // st["nbuckets"] == SLOTS[ngenomes], st
        _export_equals(tbl, dbs, (n, ngenomes))
        assert st["nkeys"] == nkeys
    finally:
        tbl.close()


@pytest.mark.parametrize("ends_empty", [True, False])
def test_build_ending_on_an_empty_run_and_on_a_contig_with_kmers(ctx, ends_empty):
    genomes, dbs = case(3, K, 2049, ends_empty)
    assert (len(genomes[0][-1]) < K) == ends_empty
    tbl = _build(ctx, genomes, K, _nkeys(dbs))
    try:
        _export_equals(tbl, dbs, ends_empty)
        assert tbl.stats()["nkeys"] == _nkeys(dbs)
    finally:
        tbl.close()


@pytest.mark.parametrize("n", mc.COUNTS)
def test_per_thread_build_gives_the_same_set(ctx, n, monkeypatch):
    """PG_INSERT_PER_THREAD=1: one launch per contig with a k-mer instead of one over tile0"""
    genomes, dbs = case(3, K, n)
    monkeypatch.setenv("PG_INSERT_PER_THREAD", "1")
    tbl = _build(ctx, genomes, K, _nkeys(dbs))
    try:
        _export_equals(tbl, dbs, n)
        assert tbl.stats()["nkeys"] == _nkeys(dbs)
    finally:
        tbl.close()


@functools.lru_cache(maxsize=None)
def regrowth_sets(repeats=False):
    """three genomes of 10, 1024 and 2051 contigs, diverged copies of one sequence; ``repeats``: each genome is a sequence and a
    diverged copy of it back to back, so that k-mers occur twice in it"""
    tile = _tile()
    totals = [mc.total_bases(K, n, SEED, tile) for n in mc.REGROWTH]
    gen = po.synth_genomes(4, [max(totals)], 0.02, SEED + 1)
    out = []
    for g, (n, total) in enumerate(zip(mc.REGROWTH, totals)):
        codes = gen[g][0]
        if repeats:
            half = (total + 1) // 2
            codes = np.concatenate([gen[g][0][:half], gen[g + 1][0][:half]])
        out.append(mc.fragments(codes, K, n, SEED, tile))
    return out


@pytest.mark.parametrize("how", ["insert", "update", "min_count"])
def test_tile0_is_regrown_twice_in_one_table(ctx, how):
    """sets of 10, 1024 and 2051 contigs into ONE table, in this order: tile0 has room for 1024 words after the first, needs 1025
    for the second (regrown to 2050) and 2052 for the third (regrown again).  After each step the table holds the oracle's set:
    by insert_seqset; by update_seqset (the first genome's keys, the masks of all); by insert_seqset(min_count=2)."""
    from panagram_amd import engine
    sets = regrowth_sets(repeats=(how == "min_count"))
    assert [len(s) for s in sets] == [10, 1024, 2051]
    tbl = engine.PanTable(ctx, K, 3)
    try:
        for g in range(3):
            ss = engine.SeqSet.from_host(ctx, sets[g])
            if how == "insert" or (how == "update" and g == 0):
                tbl.insert_seqset(g, ss)
            elif how == "update":
                tbl.update_seqset(g, ss)
            else:
                tbl.insert_seqset(g, ss, min_count=2)
            ss.close()
            so_far = [sets[x] if x <= g else [] for x in range(3)]
            if how == "min_count":
                fk, fm = po.build_bitvec_dbs(so_far, K, min_counts=[2, 2, 2])[0]
                assert len(fk) > 100 * (g + 1)
            else:
                fk, fm = po.build_bitvec_dbs(so_far, K)[0]
            if how == "update":  # the first genome's keys alone
                own = np.isin(fk, po.build_bitvec_dbs([sets[0]], K)[0][0])
                fk, fm = fk[own], fm[own]
                assert g == 0 or (fm != 1).sum() > 1000
            _export_equals(tbl, [(fk, fm)], (how, g))
            assert tbl.stats()["nkeys"] == len(fk), (how, g)
    finally:
        tbl.close()


# ---------------------------------------------------------------------------
# anchoring
# ---------------------------------------------------------------------------
ANCHOR_CASES = [(3, 21, 3000), (40, 31, 3000), (100, 21, 1025), (130, 21, 1025)]  # k_epilogue_b1, _n, _w, _chunks


@pytest.fixture(scope="module")
def anchored(ctx):
    """(table, sequence set of g0, oracle per contig) per case, built once"""
    from panagram_amd import engine
    made = {}

    def get(ngenomes, k, n):
        if (ngenomes, k, n) not in made:
            genomes, dbs = case(ngenomes, k, n)
            made[(ngenomes, k, n)] = (_build(ctx, genomes, k, _nkeys(dbs)), engine.SeqSet.from_host(ctx, genomes[0]), contig_oracle(ngenomes, k, n))
        return made[(ngenomes, k, n)]
    yield get
    for tbl, ss, _ in made.values():
        ss.close()
        tbl.close()


def _poison(res):
    """0xAA into every byte of the result's row buffer (on the context's stream, ahead of the run): a closed result's buffer
    is kept for the next one of its size, so the rows of an earlier run would still be there — what is compared afterwards
    was written by the run under test"""
    import ctypes as C
    from panagram_amd.engine import check
    (ptr, size), _ = res.device_ptrs()
    check(res.ctx._lib.pg_device_memset(res.ctx._h, C.c_void_p(ptr), 0xAA, size))


def _check_rows(res, oracle, tag, contigs=None, stats=False):
    ccs = res.contig_colsums().astype(np.int64) if stats else None
    for i in (range(len(oracle)) if contigs is None else contigs):
        rows, rows100, bins, info = res.download(i, want_bitmap100=stats)
        if oracle[i] is None:
            assert rows.shape[0] == 0 and info["nkmers"] == 0, (tag, i)
            continue
        o_rows, o_rows100, o_bins, o_cs = oracle[i]
        assert rows.shape == o_rows.shape and np.array_equal(rows, o_rows), (tag, i)
        if stats:
            assert np.array_equal(rows100, o_rows100), (tag, i)
            assert np.array_equal(bins.astype(np.int64), o_bins), (tag, i)
            assert np.array_equal(ccs[i], o_cs), (tag, i)


@pytest.mark.parametrize("ngenomes,k,n", ANCHOR_CASES)
def test_anchor_every_contig_against_the_oracle(anchored, ngenomes, k, n):
    """rows, low-resolution rows, bins and column sums of EVERY contig; the contigs without a k-mer have no row"""
    from panagram_amd import engine
    tbl, ss, oracle = anchored(ngenomes, k, n)
    res = engine.AnchorResult(tbl, ss, colsums=True)
    try:
        _poison(res)
        res.run()
        _check_rows(res, oracle, "run", stats=True)
        total = np.sum([o[3] for o in oracle if o is not None], axis=0)
        assert np.array_equal(res.colsums().astype(np.int64), total)
    finally:
        res.close()


@pytest.mark.parametrize("ngenomes,k,n", ANCHOR_CASES)
def test_contigs_small_over_all_and_over_a_range_between_empty_runs(anchored, ngenomes, k, n):
    from panagram_amd import engine
    tbl, ss, oracle = anchored(ngenomes, k, n)
    res = engine.AnchorResult(tbl, ss, colsums=True)
    try:
        _poison(res)
        res.run()
        m0, _ = mc.middle_run(n)
        for first, count in ((0, n), (2, m0 + 5 - 2), (m0 + 3, n - 3 - (m0 + 3))):  # from inside an empty run to inside the next
            assert oracle[first] is None and oracle[first + count - 1] is None
            small = res.contigs_small(first, count)
            assert len(small) == count
            for j in range(count):
                _, _, bins, info = small[j]
                o = oracle[first + j]
                if o is None:
                    assert info["nkmers"] == 0 and info["nbins"] == 0 and len(bins) == 0, (first, j)
                    continue
                assert info["nkmers"] == len(o[0]) and info["nrows100"] == len(o[1]) and info["nbins"] == len(o[2]), (first, j)
                assert info["binlen"] == max(1, po.bin_length(len(o[0]))), (first, j)
                assert np.array_equal(bins.astype(np.int64), o[2]), (first, j)
    finally:
        res.close()


def _range_cases(oracle, n):
    """(first contig, count): one starting at a contig without k-mers, one ending at such a contig, one of a single one-k-mer
    contig"""
    m0, mn = mc.middle_run(n)
    one = next(i for i, o in enumerate(oracle) if o is not None and len(o[0]) == 1)
    cases = [(m0 + mn - 2, 40), (m0 - 40, 40 + 3), (one, 1)]
    assert oracle[cases[0][0]] is None and oracle[cases[0][0] + 39] is not None      # starts inside the run of empty contigs
    assert oracle[cases[1][0]] is not None and oracle[cases[1][0] + 42] is None      # ends inside it
    return cases


@pytest.mark.parametrize("ngenomes,k,n", ANCHOR_CASES)
def test_rows_only_and_run_range(anchored, ngenomes, k, n):
    """search's mode (rows only) gives the same rows; run_range over a range of a fresh result gives the whole run's rows of
    those contigs"""
    from panagram_amd import engine
    tbl, ss, oracle = anchored(ngenomes, k, n)
    res = engine.AnchorResult(tbl, ss, colsums=False, rows_only=True)
    try:
        _poison(res)
        res.run()
        _check_rows(res, oracle, "rows only")
    finally:
        res.close()
    for first, count in _range_cases(oracle, n):
        res = engine.AnchorResult(tbl, ss, colsums=False, rows_only=True)
        try:
            _poison(res)
            res.run_range(first, count)
            _check_rows(res, oracle, ("range", first, count), contigs=range(first, first + count))
        finally:
            res.close()


@pytest.mark.parametrize("piece", [0, 1])
@pytest.mark.parametrize("ngenomes,k,n", ANCHOR_CASES[:2])
def test_coschedule_of_three_interleaved_groups(anchored, ngenomes, k, n, piece):
    from panagram_amd import engine
    tbl, ss, oracle = anchored(ngenomes, k, n)
    res = engine.AnchorResult(tbl, ss, colsums=True)
    try:
        res.coschedule(np.arange(n, dtype=np.uint32) % 3, piece_tiles=piece)
        _poison(res)
        res.run()
        _check_rows(res, oracle, ("coscheduled", piece), stats=True)
    finally:
        res.close()


def test_write_bgzf_of_every_contigs_rows(anchored, tmp_path):
    from panagram_amd import engine
    tbl, ss, oracle = anchored(*ANCHOR_CASES[0])
    res = engine.AnchorResult(tbl, ss, colsums=True)
    try:
        _poison(res)
        res.run()
        for step, which in ((1, 0), (100, 1)):
            path = str(tmp_path / f"bitmap.{step}.gz")
            res.write_bgzf(step, path, path + ".gzi")
            with gzip.open(path, "rb") as f:
                got = f.read()
            assert got == b"".join(o[which].tobytes() for o in oracle if o is not None), step
    finally:
        res.close()


# ---------------------------------------------------------------------------
# FASTA text with many records
# ---------------------------------------------------------------------------
def _read_fasta(tmp_path, text):
    from panagram_amd import index as pidx
    p = tmp_path / "x.fa"
    p.write_bytes(text)
    return list(pidx.read_fasta(str(p)))


@pytest.mark.parametrize("width,crlf", [(1, False), (7, False), (60, False), (60, True)])
def test_fasta_of_the_fragmented_set(ctx, tmp_path, width, crlf):
    """3000 records, the empty ones among them, in lines of 1, 7 and 60 bases (a small text: the host looks for the headers):
    names and lengths are index.read_fasta's, every record unpacks to its bases"""
    from panagram_amd import engine
    contigs = case(3, K, 3000)[0][0]
    text = mc.fasta(contigs, width, crlf)
    recs = _read_fasta(tmp_path, text)
    ss = engine.SeqSet.from_fasta(ctx, text)
    try:
        assert list(ss.names) == [r[0] for r in recs] == mc.names_for(3000)
        assert np.asarray(ss.lens, np.int64).tolist() == [len(r[1]) for r in recs]
        for i, (_, seq) in enumerate(recs):
            assert ss.unpack(i) == mc.norm(seq), i
    finally:
        ss.close()


@pytest.mark.parametrize("nheaders", mc.HEADER_COUNTS)
def test_fasta_with_header_lines_around_the_device_lists_capacity(ctx, tmp_path, nheaders, monkeypatch):
    """a text of more than 4 MB with 65535, 65536 and 65537 header lines (the device's list holds 65536 positions; past that
    the host scans for itself): names and lengths of all records, the bases of more than 2000 of them, and the same answer with
    the host's scan forced"""
    from panagram_amd import engine
    text, _, _ = mc.header_text(nheaders, 11)
    names, lens, offs = search.scan_fasta(text)
    recs = _read_fasta(tmp_path, text)
    assert len(text) >= mc.BIG_TEXT and len(recs) == nheaders
    assert [r[0] for r in recs] == names and [len(r[1]) for r in recs] == lens.tolist()
    pick = mc.header_text_picks(text, offs, lens)
    assert len(pick) >= 2000
    monkeypatch.delenv("PG_FASTA_HOST_SCAN", raising=False)
    answers = []
    for host_scan in (False, True):
        if host_scan:
            monkeypatch.setenv("PG_FASTA_HOST_SCAN", "1")
        ss = engine.SeqSet.from_fasta(ctx, text)
        try:
            assert list(ss.names) == names, host_scan
            assert np.array_equal(np.asarray(ss.lens, np.int64), lens), host_scan
            got = [ss.unpack(i) for i in pick]
            assert got == [mc.norm(recs[i][1]) for i in pick], host_scan
            answers.append((list(ss.names), np.asarray(ss.lens, np.int64).tolist(), got))
        finally:
            ss.close()
    assert answers[0] == answers[1]


# ---------------------------------------------------------------------------
# search with many queries
# ---------------------------------------------------------------------------
NQUERIES = 3000


@functools.lru_cache(maxsize=None)
def search_case():
    """(genomes, k, [(name, sequence)]): segments of 25 to 400 bases of the three genomes of tests/test_gpu_search_e2e.py, every
    fifth reverse-complemented, every seventh with an N, every eleventh random, every thirteenth (and the first and the last
    three) shorter than k"""
    from tests import test_gpu_search_e2e as e2e
    genomes, k = e2e._genomes(), e2e.K
    rng = np.random.default_rng(21)
    out = []
    for i in range(NQUERIES):
        g = genomes[i % 3]
        n = int(rng.integers(25, 401))
        at = int(rng.integers(0, len(g) - n))
        seq = g[at:at + n]
        if i % 11 == 4:
            seq = po.codes_to_ascii(rng.integers(0, 4, n, dtype=np.uint8))
        if i % 5 == 2:
            seq = e2e._revcomp(seq)
        if i % 7 == 3:
            seq = seq[:n // 2] + b"N" + seq[n // 2 + 1:]
        if i % 13 == 6 or i == 0 or i >= NQUERIES - 3:
            seq = seq[:int(rng.integers(0, k))]
        out.append((f"q{i}", seq))
    return genomes, k, out


def _same_frames(got, want, tag):
    for g, w, what in zip(got, want, ("long", "matrix", "summary")):
        g, w = (g.reset_index(), w.reset_index()) if what == "matrix" else (g, w)
        assert list(g.columns) == list(w.columns) and len(g) == len(w), (tag, what)
        for col in w.columns:
            assert g[col].tolist() == w[col].tolist(), (tag, what, col)


def test_search_with_three_thousand_queries(ctx, tmp_path_factory):
    """one record and one presence-profile window per query: the frames are the model's on the oracle's rows, whether all
    records go in one batch (queries shorter than k among them: the records are picked out), one record per batch, or about
    1100 per batch"""
    from panagram_amd import index as pidx
    from tests import test_gpu_search_e2e as e2e
    genomes, k, queries = search_case()
    tmp = tmp_path_factory.mktemp("many_queries")
    lines = ["name\tfasta"]
    for i, seq in enumerate(genomes):
        fa = tmp / f"g{i}.fa"
        fa.write_bytes(po.fasta_text(["chr1"], [seq]))
        lines.append(f"g{i}\t{fa}")
    (tmp / "samples.tsv").write_text("\n".join(lines) + "\n")
    out = str(tmp / "idx")
    pidx.Index(str(tmp / "samples.tsv"), prefix=out, k=k, anchor_genomes=["g0"], lowres_step=100).run()
    dbs = po.build_bitvec_dbs([[g] for g in genomes], k)
    prof, allnone = [], []
    for _, seq in queries:
        masks = po.counters_for_read(dbs[0], seq, k)
        bits = ((masks[:, None] >> np.arange(3, dtype=np.uint32)[None, :]) & 1).astype(np.uint8)
        p, an = search_ref.ref_window(bits, k)
        prof.append(p)
        allnone.append(an)
    names, lens = [q[0] for q in queries], [len(q[1]) for q in queries]
    want = search.frames(names, lens, k, e2e.NAMES, np.stack(prof), np.array(allnone, np.int64))
    short = sum(n < k for n in lens)
    assert short > 200 and lens[0] < k and all(n < k for n in lens[-3:]) and want[2]["best"].nunique() == 4
    per_batch = sum(lens) * 1100 // NQUERIES
    assert [len(search.batches(lens, b)) for b in (search.BATCH_BASES, per_batch, 1)] == [1, 3, NQUERIES]
    idx = pidx.Index(out, mode="r")
    try:
        got = idx.search(queries)
        _same_frames(got, want, "one batch")
        for batch_bases in (1, per_batch):
            again = idx.search(queries, batch_bases=batch_bases)
            _same_frames(again, want, batch_bases)
            assert all(a.equals(b) for a, b in zip(again, got)), batch_bases
    finally:
        idx.close()


# ---------------------------------------------------------------------------
# the other per-contig arrays
# ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def frag(ctx):
    """(contigs, sequence set) of the 3000-contig genome"""
    from panagram_amd import engine
    contigs = case(3, K, 3000)[0][0]
    ss = engine.SeqSet.from_host(ctx, contigs)
    yield contigs, ss
    ss.close()


def _same_set(ss, contigs, tag):
    assert np.asarray(ss.lens, np.int64).tolist() == [len(c) for c in contigs], tag
    for i, c in enumerate(contigs):
        assert ss.unpack(i) == mc.norm(c), (tag, i)


def test_concat_concat_ranges_and_slice(ctx, frag):
    from panagram_amd import engine
    contigs, ss = frag
    _same_set(ss, contigs, "from_host")
    cuts = [(0, 1100), (1100, 2200), (1900, 3000)]
    parts = [engine.SeqSet.from_host(ctx, contigs[a:b]) for a, b in cuts]
    made = []
    try:
        cat = engine.SeqSet.concat(ctx, parts)
        made.append(cat)
        assert len(cat.lens) == 3300
        _same_set(cat, [c for a, b in cuts for c in contigs[a:b]], "concat")
        # ranges that begin and end on contigs without a k-mer: the front run to the middle run, the middle run to the end run,
        # a range of empty contigs alone, and the first range again
        m0, mn = mc.middle_run(3000)
        ranges = [(ss, 1, m0 + 4), (ss, m0 + 2, 3000 - 2 - (m0 + 2)), (ss, m0, mn), (parts[2], 1100 - 4, 3), (ss, 1, m0 + 4)]
        for s, first, count in ranges:
            assert s.lens[first] < K and s.lens[first + count - 1] < K
        cr = engine.SeqSet.concat_ranges(ctx, ranges)
        made.append(cr)
        _same_set(cr, [c for s, first, count in ranges for c in (contigs if s is ss else contigs[1900:3000])[first:first + count]], "concat_ranges")
        # 2000 pieces, starts on 32-base words
        pieces = []
        for c, seq in enumerate(contigs):
            n = len(seq)
            for start in range(0, n, 32 * max(1, n // 256)):
                pieces.append((c, start, min(n - start, 1 + (7 * start + c) % 97)))
        assert len(pieces) > 2000
        pieces = pieces[::len(pieces) // 2000][:2000]
        assert len(pieces) == 2000 and len({p[0] for p in pieces}) > 600 and max(p[1] for p in pieces) > 10000
        sl = ss.slice(pieces)
        made.append(sl)
        _same_set(sl, [contigs[c][s0:s0 + n] for c, s0, n in pieces], "slice")
    finally:
        for x in made + parts:
            x.close()


def test_kmer_sketch_registers(ctx, frag):
    from panagram_amd import engine
    contigs, ss = frag
    sk = engine.KmerSketch(ctx, K)
    try:
        sk.add(ss)
        assert np.array_equal(sk.registers(), po.sketch_registers(contigs, K))
    finally:
        sk.close()


def test_minhash_sketch_and_bases(ctx, frag):
    from panagram_amd import engine
    contigs, ss = frag
    mh = engine.MinHashSketch(ctx)
    try:
        mh.add(ss)
        got, bases = mh.result()
        assert np.array_equal(got, minhash_ref.sketch(contigs)) and bases == minhash_ref.acgt_bases(contigs)
    finally:
        mh.close()


WIDE = dict(min_run=1, max_gap=1000, max_shift=100)


@functools.lru_cache(maxsize=None)
def synteny_model(frag_is_a):
    genomes = case(3, K, 3000)[0]
    a, b = (genomes[0], genomes[1]) if frag_is_a else (genomes[1], genomes[0])
    m, nk = sr.mates(a, b, K)
    runs = sr.runs(m, nk)
    lens_b = np.array([len(c) for c in b], np.int64)
    return a, b, m, nk, runs, br.blocks(runs, lens_b, **WIDE), vr.variants(runs, a, b, K, **WIDE)


@pytest.mark.parametrize("frag_is_a", [True, False])
def test_synteny_of_the_fragmented_set_and_its_whole_copy(ctx, frag, frag_is_a):
    """the fragmented genome against its whole diverged copy and the other way round: mates, runs, blocks and variants and
    their counts per contig are the models'"""
    from panagram_amd import engine
    a, b, m, nk, runs, blocks, var = synteny_model(frag_is_a)
    whole = engine.SeqSet.from_host(ctx, case(3, K, 3000)[0][1])
    ssa, ssb = (frag[1], whole) if frag_is_a else (whole, frag[1])
    try:
        pt = engine.PosTable(ctx, K, max(1, ssa.total_kmers(K) + ssb.total_kmers(K)))
        try:
            pt.insert(0, ssa)
            pt.insert(1, ssb)
            got, nmated = pt.mates(ssa)
        finally:
            pt.close()
        assert np.array_equal(got, m) and nmated == int((m != sr.NO_MATE).sum()) > 100_000
        ncontigs = len(a)
        rc, rs, re_, rm, per, nmated = engine.synteny_segments(ctx, K, ssa, ssb)
        assert np.array_equal(np.stack([rc, rs, re_, rm], axis=1).astype(np.int64), runs) and len(runs) > 2000
        assert np.array_equal(per.astype(np.int64), np.bincount(runs[:, 0], minlength=ncontigs)[:ncontigs])
        blk = engine.synteny_blocks(ctx, K, ssa, ssb, **WIDE)
        assert np.array_equal(np.stack(blk[:8], axis=1).astype(np.int64), blocks)
        assert np.array_equal(blk[8].astype(np.int64), np.bincount(blocks[:, 0], minlength=ncontigs)[:ncontigs])
        assert blk[9:] == (nmated, len(runs))
        got = engine.synteny_variants(ctx, K, ssa, ssb, **WIDE)
        assert np.stack(got[:7], axis=1).astype(np.int64).tolist() == var["records"].tolist()
        assert np.stack(got[7:9], axis=1).tolist() == var["words"].tolist()
        assert got[9].astype(np.int64).tolist() == var["classes"] and got[10] == var["links"]
        assert got[11:] == (nmated, len(runs), len(blocks)) and len(var["records"]) > 500
    finally:
        whole.close()
