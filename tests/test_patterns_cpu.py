"""CPU: the numpy restatement of the pattern spectrum (tests/patterns_ref.py) against DataFrame.value_counts(), the host side
of Genome.pattern_spectrum (panagram_amd/patterns.py), the chunk constant, and the `patterns` subcommand's argument errors."""
import os
import re

import numpy as np
import pandas as pd
import pytest

from panagram_amd import patterns
from tests import rows_craft as rc
from tests.patterns_ref import ref_keys, ref_pattern_counts

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("n,select", [(1, [0]), (8, list(range(8))), (9, [0, 8]), (9, list(range(9))), (33, [31, 32]),
                                      (33, [0, 5, 17, 31, 32])])
def test_reference_equals_value_counts(n, select):
    rng = np.random.default_rng(11 + n)
    rows = [rc.pack(rng.random((700, n)) < 0.3), rc.pack(rng.random((90, n)) < 0.7)]
    contigs, starts, ends = [0, 1, 0, 1], [0, 3, 10, 0], [700, 90, 55, 0]
    for stride in (1, 3):
        ns = [(len(r) - 1) // stride + 1 for r in rows]
        e = [min(b, ns[c]) for c, b in zip(contigs, ends)]
        keys, counts, total = ref_pattern_counts(rows, n, contigs, starts, e, stride, select)
        frames = [pd.DataFrame(rc.unpack(rows[c], n)[::stride][a:b][:, select]) for c, a, b in zip(contigs, starts, e)]
        vc = pd.concat(frames, ignore_index=True).value_counts()
        want = {sum(int(b) << i for i, b in enumerate(pat)): int(v) for pat, v in vc.items()}
        assert dict(zip(keys.tolist(), counts.tolist())) == want
        assert keys.dtype == np.uint64 and (np.diff(keys.astype(object)) > 0).all()
        assert total == int(counts.sum()) == sum(b - a for a, b in zip(starts, e))


def test_reference_keys_by_hand():
    rows = rc.pack([[1, 0, 1, 0, 0, 0, 0, 0, 1], [0, 1, 1, 0, 0, 0, 0, 0, 0], [1, 1, 1, 1, 1, 1, 1, 1, 1]])
    assert ref_keys(rows, 9, 1, range(9)).tolist() == [0b100000101, 0b110, 0b111111111]
    assert ref_keys(rows, 9, 1, [0, 8]).tolist() == [0b11, 0b00, 0b11]
    assert ref_keys(rows, 9, 2, [8, 1]).tolist() == [0b10, 0b11]  # (column order, not the order given)
    assert ref_keys(rc.ones(2, 64), 64, 1, range(64)).tolist() == [2 ** 64 - 1] * 2
    # bits past N in the last byte are no part of a key
    assert ref_keys(rc.with_pad_bits(rows, 9), 9, 1, range(9)).tolist() == [0b100000101, 0b110, 0b111111111]


def test_select_words():
    names = [f"g{i}" for i in range(70)]
    w, sel = patterns.select_words(names, ["g69", "g0", 33])
    assert w.dtype == np.uint32 and w.tolist() == [1, 2, 1 << 5] and sel == ["g0", "g33", "g69"]
    w, sel = patterns.select_words(names[:9])
    assert w.tolist() == [0x1FF] and sel == names[:9]
    w, sel = patterns.select_words(names[:64], None)
    assert w.tolist() == [0xFFFFFFFF, 0xFFFFFFFF] and len(sel) == 64
    w, sel = patterns.select_words(names, range(3, 67))
    assert len(sel) == 64 and int(sum(bin(int(x)).count("1") for x in w)) == 64
    with pytest.raises(ValueError, match="'zz'"):
        patterns.select_words(names, ["g1", "zz"])
    with pytest.raises(ValueError, match="twice"):
        patterns.select_words(names, ["g1", 1])
    with pytest.raises(ValueError, match="out of range"):
        patterns.select_words(names, [70])
    with pytest.raises(ValueError, match="out of range"):
        patterns.select_words(names, [-1])
    with pytest.raises(ValueError, match="no genome"):
        patterns.select_words(names, [])
    with pytest.raises(ValueError, match="at most 64"):
        patterns.select_words(names)
    with pytest.raises(ValueError, match="65 genomes"):
        patterns.select_words(names, range(65))


def test_merge():
    z = np.zeros(0, np.uint64)
    k, c = patterns.merge([])
    assert k.dtype == np.uint64 and c.dtype == np.uint64 and len(k) == 0 and len(c) == 0
    top = 2 ** 64 - 1
    k, c = patterns.merge([([1, 5, top], [10, 20, 30]), (z, z), ([0, 5], [1, 2]), ([top], [7])])
    assert k.tolist() == [0, 1, 5, top] and c.tolist() == [1, 10, 22, 37] and k.dtype == np.uint64 and c.dtype == np.uint64
    rng = np.random.default_rng(2)
    parts = [(np.unique(rng.integers(0, 50, 30)).astype(np.uint64),) for _ in range(5)]
    parts = [(p[0], rng.integers(1, 10 ** 9, len(p[0])).astype(np.uint64)) for p in parts]
    want = {}
    for pk, pc in parts:
        for a, b in zip(pk.tolist(), pc.tolist()):
            want[a] = want.get(a, 0) + b
    k, c = patterns.merge(parts)
    assert dict(zip(k.tolist(), c.tolist())) == want and k.tolist() == sorted(want)
    with pytest.raises(ValueError):
        patterns.merge([([1, 2], [1])])


def test_spectrum_frame_order_ties_and_frac():
    names = ["a", "b", "c"]
    keys, counts = [0b000, 0b001, 0b110, 0b111, 0b100], [5, 40, 40, 10, 5]
    f = patterns.spectrum_frame(keys, counts, names)
    assert list(f.columns) == ["pattern", "n", "rows", "frac"]
    # rows descending; ties by pattern ascending ("011" < "100": key 0b110 is a = 0, b = 1, c = 1)
    assert f["pattern"].tolist() == ["011", "100", "111", "000", "001"]
    assert f["n"].tolist() == [2, 1, 3, 0, 1] and f["rows"].tolist() == [40, 40, 10, 5, 5]
    assert np.allclose(f["frac"], np.array([40, 40, 10, 5, 5]) / 100) and f["rows"].dtype == np.int64
    # frac is taken over the uncut total
    g = patterns.spectrum_frame(keys, counts, names, top=2)
    assert g["pattern"].tolist() == ["011", "100"] and g["frac"].tolist() == [0.4, 0.4]
    g = patterns.spectrum_frame(keys, counts, names, min_rows=10)
    assert g["pattern"].tolist() == ["011", "100", "111"] and g["frac"].tolist() == [0.4, 0.4, 0.1]
    g = patterns.spectrum_frame(keys, counts, names, top=1, min_rows=6)
    assert g["pattern"].tolist() == ["011"] and list(g.index) == [0]
    assert len(patterns.spectrum_frame(keys, counts, names, top=0)) == 0
    e = patterns.spectrum_frame([], [], names)
    assert list(e.columns) == ["pattern", "n", "rows", "frac"] and len(e) == 0
    # 64 genomes: the all-ones key
    f = patterns.spectrum_frame([2 ** 64 - 1, 1 << 63], [3, 1], [f"g{i}" for i in range(64)])
    assert f["pattern"].tolist() == ["1" * 64, "0" * 63 + "1"] and f["n"].tolist() == [64, 1]
    for bad in (dict(top=-1), dict(min_rows=-1)):
        with pytest.raises(ValueError):
            patterns.spectrum_frame(keys, counts, names, **bad)
    with pytest.raises(ValueError, match="bits at or past"):
        patterns.spectrum_frame([0b1000], [1], names)
    with pytest.raises(ValueError):
        patterns.spectrum_frame([1, 2], [1], names)
    with pytest.raises(ValueError):
        patterns.spectrum_frame([], [], [])


def test_occupancy():
    occ = patterns.occupancy([0b000, 0b001, 0b110, 0b111, 0b100], [5, 40, 40, 10, 5], 3)
    assert occ.dtype == np.int64 and occ.tolist() == [5, 45, 40, 10]
    assert patterns.occupancy([], [], 5).tolist() == [0] * 6
    assert patterns.occupancy([2 ** 64 - 1], [9], 64).tolist() == [0] * 64 + [9]
    with pytest.raises(ValueError):
        patterns.occupancy([4], [1], 2)
    with pytest.raises(ValueError):
        patterns.occupancy([], [], 65)


def test_chunk_constant_is_the_kernels():
    from panagram_amd import engine
    txt = open(os.path.join(ROOT, "panagram_amd", "csrc", "pg_kernels.h")).read()
    assert int(re.search(r"constexpr uint32_t PATTERN_CHUNK = (\d+);", txt).group(1)) == engine.PATTERN_CHUNK
    assert engine.PATTERN_CHUNK % 256 == 0 and 0 < engine.PATTERN_FIRST_CAP <= engine.PATTERN_MAX_CAP
    assert hasattr(engine.AnchorResult, "pattern_counts")


@pytest.mark.parametrize("args,msg", [
    (["/no/such/index", "g0"], "give a chromosome or --whole"),
    (["/no/such/index", "g0", "chr1", "--whole"], "give a chromosome or --whole"),
    (["/no/such/index", "g0", "chr1", "--occupancy", "--top", "3"], "--occupancy takes no"),
    (["/no/such/index", "g0", "chr1", "--top", "-1"], "must not be negative"),
    (["/no/such/index", "g0", "chr1", "--min-rows", "-2"], "must not be negative"),
    (["/no/such/index", "g0", "chr1", "0", "ten"], "invalid int value")])
def test_cli_argument_errors_exit_before_any_index_is_opened(args, msg, capsys, monkeypatch):
    from panagram_amd import __main__ as cli
    from panagram_amd import index as pidx

    def no_index(*a, **k):
        raise AssertionError("an index was opened")
    monkeypatch.setattr(pidx, "Index", no_index)
    with pytest.raises(SystemExit) as ei:
        cli.main(["patterns"] + args)
    assert ei.value.code == 2 and msg in capsys.readouterr().err
