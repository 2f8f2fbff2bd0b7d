"""CPU: what the four readers of bitmap rows — Genome.pair_counts, find_pattern, kmer_similarity_bins, pattern_density —
share: a rows container is closed when the engine call on it raises, and before the next one is opened (a container holds
up to similarity_budget bytes of HBM), and their argument checks refuse in one order, before anything is read.  With
test_find_pattern_cpu.py's scene and stand-in containers that count their close() calls."""
from types import SimpleNamespace

import numpy as np
import pytest

from tests import rows_craft as rc
from tests import test_find_pattern_cpu as fp
from tests.pairs_ref import ref_pair_counts

RULE = (["g1"], ["g2"], None, 0)


class _Boom(Exception):
    pass


class _Rows(fp._Rows):
    """test_find_pattern_cpu's stand-in, with the two reductions it lacks"""

    def pair_counts(self, contigs, starts, ends, step, stride):
        assert step == self.bstep
        return np.stack([ref_pair_counts(self.rows[c], self.n, s, e, stride) for c, s, e in zip(contigs, starts, ends)]).astype(np.uint64)

    def bin_colsums(self, contigs, starts, ends, step, stride, keep_words, omit_fixed):
        assert step == self.bstep
        parts = [rc.ref_bin_colsums(self.rows[c], self.n, [s], [e], stride, keep_words, omit_fixed) for c, s, e in zip(contigs, starts, ends)]
        return np.concatenate([p[0] for p in parts]).astype(np.uint64), np.concatenate([p[1] for p in parts]).astype(np.uint64)


class _Watched:
    """a stand-in container that books its opening and its close() calls, and whose engine calls count towards book.fail_at"""

    def __init__(self, inner, book):
        assert all(w.closed for w in book.opened), "a container is opened while another one is still open"
        self._inner, self._book, self.closed = inner, book, 0
        book.opened.append(self)

    def __getattr__(self, name):
        fn = getattr(self._inner, name)

        def call(*args, **kw):
            self._book.calls += 1
            if self._book.calls == self._book.fail_at:
                raise _Boom(name)
            return fn(*args, **kw)
        return call

    def close(self):
        self.closed += 1


def _watched_scene(monkeypatch, fail_at=None, n=11):
    idx, g, log = fp._find_scene(monkeypatch, n)
    book = SimpleNamespace(opened=[], calls=0, fail_at=fail_at)
    region, disk = g._rows_region, g._rows_from_disk

    def watched(r):
        return _Watched(_Rows(r.rows, n, r.bstep), book)
    g._rows_region = lambda bstep, row0, nrows: watched(region(bstep, row0, nrows))
    g._rows_from_disk = lambda chroms, step=1: watched(disk(chroms, step))
    return g, book


# (reader, arguments that make it open at least three containers under a budget of 50 rows)
READS = [("pair_counts", ("c1", 3, 1230, 7)),
         ("find_pattern", RULE + ("c1", 3, 1230, 7)),
         ("kmer_similarity_bins", (None, 7, 100)),
         ("pattern_density", RULE + (None, 7, 100))]


@pytest.mark.parametrize("reader,args", READS)
def test_a_failing_engine_call_closes_its_container(monkeypatch, reader, args):
    """the engine call on the second container raises: the caller sees that exception, both containers have been closed
    once by then (the exception and its traceback still alive), and no third one is opened"""
    g, book = _watched_scene(monkeypatch, fail_at=2)
    g.similarity_budget = 50 * g.nbytes
    with pytest.raises(_Boom) as caught:
        getattr(g, reader)(*args)
    assert caught.tb is not None
    assert book.calls == 2 and len(book.opened) == 2
    assert [w.closed for w in book.opened] == [1, 1]


@pytest.mark.parametrize("reader,args", READS)
def test_a_container_is_closed_before_the_next_is_opened(monkeypatch, reader, args):
    """c1 in pieces of at most 50 rows at step 7, every chromosome a batch of its own: never two containers open (_Watched's
    constructor asserts it), every one closed once, and the result is the uncut one"""
    g, book = _watched_scene(monkeypatch)
    want = getattr(g, reader)(*args)
    uncut = len(book.opened)
    g.similarity_budget = 50 * g.nbytes
    got = getattr(g, reader)(*args)
    assert len(book.opened) - uncut >= 3 and book.calls == len(book.opened)
    assert [w.closed for w in book.opened] == [1] * len(book.opened)
    if isinstance(want, dict):
        assert list(got) == list(want) and all(got[c].equals(want[c]) for c in want)
    else:
        assert got.equals(want)


# every line holds two faults; the one named is the one that is reported
REFUSALS = [
    ("pair_counts", dict(chrom="nope", step=0), ValueError, "step must be positive"),
    ("find_pattern", dict(have=["g1"], chrom="nope", step=0), ValueError, "step must be positive"),
    ("kmer_similarity_bins", dict(chroms=["nope"], step=0), ValueError, "step and bin_size must be positive"),
    ("pattern_density", dict(have=["g1"], chroms=["nope"], step=0), ValueError, "step and bin_size must be positive"),
    ("kmer_similarity_bins", dict(chroms=["nope"], bin_size=0), ValueError, "step and bin_size must be positive"),
    ("pattern_density", dict(have=["g1"], chroms=["nope"], bin_size=0), ValueError, "step and bin_size must be positive"),
    ("pair_counts", dict(chrom=None, start=5, step=0), ValueError, "step must be positive"),
    ("find_pattern", dict(have=["nobody"], chrom=None, start=5), ValueError, "start and end need a chromosome"),
    ("find_pattern", dict(have=["nobody"], chrom=None, end=5), ValueError, "start and end need a chromosome"),
    ("find_pattern", dict(have=["g1"], chrom="nope", min_len=0), KeyError, "g0: no chromosome 'nope'"),
    ("find_pattern", dict(have=["nobody"], chrom="nope"), KeyError, "g0: no chromosome 'nope'"),
    ("find_pattern", dict(have=["nobody"], chrom="c1", min_len=0), ValueError, "'nobody'"),
    ("pattern_density", dict(have=["nobody"], chroms=["c1", "nope"]), KeyError, "g0: no chromosome 'nope'"),
    ("kmer_similarity_bins", dict(chroms=["c1", "nope"], keep=["nobody"]), KeyError, "g0: no chromosome 'nope'"),
    ("pair_counts", dict(chrom="nope", start=5, end=2), KeyError, "g0: no chromosome 'nope'"),
]


@pytest.mark.parametrize("reader,kwargs,error,message", REFUSALS)
def test_order_of_refusals(monkeypatch, reader, kwargs, error, message):
    """step (and bin_size), then "start and end need a chromosome", then the unknown chromosome, then the rule's genomes,
    then min_len / max_gap; nothing is read for any of them"""
    g, book = _watched_scene(monkeypatch, n=3)
    with pytest.raises(error) as caught:
        getattr(g, reader)(**kwargs)
    assert message in str(caught.value)
    assert book.opened == [] and book.calls == 0
