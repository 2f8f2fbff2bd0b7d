"""CPU: the numpy model of selecting columns out of finished rows (tests/subset_ref.py) against the oracle on the golden
cases, what the crafted cases of tests/test_gpu_rows_select.py promise, and the host functions of `subset` that need no GPU."""
import numpy as np
import pandas as pd
import pytest

from oracle import pyoracle as po
from tests import helpers as H
from tests import rows_craft as rc
from tests import subset_ref as sr

# (case, the kept genomes in kept order): one dropping selection, one reordering selection
GOLDEN_SELECTIONS = [("n9_k21", [0, 1, 2, 3, 5, 6, 7, 8]), ("n40_k31", [33, 2, 39, 17, 0, 8, 31, 32])]


@pytest.mark.parametrize("name, kept", GOLDEN_SELECTIONS, ids=[c for c, _ in GOLDEN_SELECTIONS])
def test_model_selection_of_oracle_rows_is_the_oracle_over_the_kept_genomes(name, kept):
    """the oracle's rows of all N genomes, selected == the oracle's rows against databases built from the kept genomes'
    sequences alone, in kept order; and the statistics recomputed from the selected rows are that oracle's"""
    fx = H.load_case(name)
    n, k = int(fx["ngenomes"]), int(fx["k"])
    dbs = H.case_dbs(fx)
    kept_dbs = po.build_bitvec_dbs([[seq for _, seq in po.parse_fasta_cpp(fx[f"fasta_{g}"].tobytes())] for g in kept], k)
    for g in [int(a) for a in fx["anchors"]][:2]:
        fasta = fx[f"fasta_{g}"].tobytes()
        want = po.anchor_fasta(kept_dbs, fasta, k, len(kept))
        got, cs = [], np.zeros(len(kept), np.int64)
        for _, seq in po.parse_fasta_cpp(fasta):
            full = po.anchor_contig(dbs, seq, k, n)[0]
            new = sr.select_rows(full, n, kept)
            _, colsums, _ = rc.ref_stats(new, len(kept), rc.bin_length(len(new)), 100)
            cs += colsums
            got.append(new.tobytes())
        assert b"".join(got) == want["bitmap1"]
        assert np.array_equal(cs, want["colsums"])


def test_model_ignores_stale_bits_and_zeroes_the_rest():
    clean = rc.dense(50, 13, 1)
    sel = [12, 0, 5]
    out = sr.select_rows(rc.with_pad_bits(clean, 13), 13, sel)
    assert np.array_equal(out, sr.select_rows(clean, 13, sel))
    bits = np.unpackbits(out, axis=1, bitorder="little")
    assert np.array_equal(bits[:, :3], rc.unpack(clean, 13)[:, sel]) and not bits[:, 3:].any()


def _apply_segments(rows, n_old, sel):
    """the kernel's arithmetic on the host: every row as little-endian 32-bit words, every segment one shift-and-mask of two
    neighbouring source words into one destination word"""
    nk, wn = len(rows), rc.row_bytes(len(sel))
    src = np.zeros((nk, 4 * ((rows.shape[1] + 3) // 4 + 1)), np.uint8)
    src[:, :rows.shape[1]] = rows
    src = src.view("<u4").astype(np.uint64)
    dst = np.zeros((nk, (wn + 3) // 4), np.uint64)
    for s, d, ln in sr.segments(sel):
        assert ln <= 32 and d // 32 == (d + ln - 1) // 32          # one destination word ...
        assert (s + ln - 1) // 32 - s // 32 <= 1                    # ... at most two neighbouring source words
        pair = src[:, s // 32] | (src[:, s // 32 + 1] << np.uint64(32))
        dst[:, d // 32] |= ((pair >> np.uint64(s % 32)) & np.uint64((1 << ln) - 1)) << np.uint64(d % 32)
    return dst.astype("<u4").view(np.uint8)[:, :wn]


def test_segments_applied_as_the_kernel_applies_them_equal_the_model():
    for n_old, n_new in sr.WIDTH_PAIRS:
        for stale in (False, True):
            rows = np.concatenate([r for r in sr.old_rows(n_old, stale) if len(r)][:6])
            for name, sel in sr.selections(n_old, n_new):
                assert np.array_equal(_apply_segments(rows, n_old, sel), sr.select_rows(rows, n_old, sel)), (n_old, n_new, name)


def test_segment_counts():
    """dropping one column: two segments and the cuts at destination word ends; a full reversal: one per column"""
    assert sr.segments(np.r_[0:4, 5:9]) == [(0, 0, 4), (5, 4, 4)]
    assert sr.segments(np.r_[0:40, 41:65]) == [(0, 0, 32), (32, 32, 8), (41, 40, 24)]
    assert len(sr.segments(np.arange(16)[::-1])) == 16
    assert sr.segments(np.arange(33)) == [(0, 0, 32), (32, 32, 1)]


def test_crafted_cases_cover_what_they_promise():
    pairs = sr.WIDTH_PAIRS
    forms = {sr.kernel_form(a) for a, _ in pairs}
    assert forms == {"b1", 1, 2, 3, 4, 5, 0}                                     # every template instance and the fallback
    assert {(rc.row_bytes(b) + 3) // 4 for _, b in pairs} >= {1, 2, 3, 4, 5, 6}  # every number of destination words
    steps = {(rc.row_bytes(a), rc.row_bytes(b)) for a, b in pairs}
    assert {(1, 1), (2, 1), (3, 2), (5, 4), (9, 8), (5, 5), (8, 1)} <= steps
    assert {(8, 7), (8, 1), (9, 8), (17, 16), (33, 32), (65, 64), (40, 38), (64, 8), (100, 96), (161, 160), (170, 161), (16, 16),
            (33, 33)} <= set(pairs)
    for edge in (16, 64, 1024):                                                  # a lane's positions, a slot, a tile
        assert {edge - 1, edge, edge + 1} <= set(sr.NKS)
    assert 0 in sr.NKS and 0 < sr.SPLIT < len(sr.NKS)
    for n_old, n_new in pairs:
        sels = dict(sr.selections(n_old, n_new))
        assert {"first", "last", "middle", "alternate", "one", "reversed", "shuffle"} <= set(sels)
        if n_old > n_new and 32 + (n_old - n_new) <= n_old:                        # (where the source has them)
            assert "at31" in sels and "at32" in sels                             # both sides of a 32-bit boundary
            assert 31 not in sels["at31"] and 32 not in sels["at32"]
        for name, sel in sels.items():
            assert len(sel) == (1 if name == "one" else n_new) and len(set(sel.tolist())) == len(sel) and sel.max() < n_old
        assert 0 not in sels["first"] and n_old - 1 not in sels["last"] or n_old == n_new
        assert list(sels["reversed"]) == sorted(sels["reversed"], reverse=True)
        if n_old == n_new:
            assert list(sels["reversed"]) == list(range(n_old))[::-1]            # the full reversal
        assert all(ln == 1 for _, _, ln in sr.segments(sels["alternate"]))
        if n_old > 33 and n_new > 32:  # a segment that crosses a source word boundary, in pairs of every form that has more than one source word
            assert any(s % 32 + ln > 32 for sel in sels.values() for s, _, ln in sr.segments(sel)), (n_old, n_new)
    # 64 -> 8: selections that leave a source word unread (the kernel does not fetch it)
    assert any(sr.needed_words(sel) == {0} for _, sel in sr.selections(64, 8))
    assert any(sr.needed_words(sel) == {0, 1} for _, sel in sr.selections(64, 8))


def test_keep_and_drop_become_a_selection():
    from panagram_amd import subset as ps
    names = ["a", "b", "c", "d"]
    assert ps.kept_names(names, keep="c,a") == ["c", "a"]
    assert ps.kept_names(names, keep=["d", "b", "a"]) == ["d", "b", "a"]
    assert ps.kept_names(names, drop="b") == ["a", "c", "d"]
    assert ps.kept_names(names, drop=["d", "a"]) == ["b", "c"]
    assert list(ps.selection(names, ["c", "a"])) == [2, 0] and ps.selection(names, ["c", "a"]).dtype == np.uint32
    for kw, match in ((dict(), "one of"), (dict(keep="a", drop="b"), "one of"), (dict(keep="a,x"), "no such sample.*x"),
                      (dict(drop="x"), "no such sample"), (dict(keep="a,b,a"), "twice.*a"), (dict(drop="b,b"), "twice"),
                      (dict(drop="a,b,c,d"), "nothing kept"), (dict(keep=""), "nothing kept")):
        with pytest.raises(ValueError, match=match):
            ps.kept_names(names, **kw)


def test_samples_table_is_renumbered_in_kept_order():
    from panagram_amd import subset as ps
    samples = pd.DataFrame({"name": ["a", "b", "c", "d"], "fasta": ["a.fa", "b.fa", "c.fa", "d.fa"],
                            "gff": [np.nan, "b.gff", np.nan, np.nan], "id": [0, 1, 2, 3], "anchor": [True, True, False, True]}).set_index("name")
    out = ps.subset_samples(samples, ["d", "b", "c"], ["d"])
    assert list(out.index) == ["d", "b", "c"] and out.index.name == "name"
    assert list(out.columns) == ["fasta", "gff", "id", "anchor"]
    assert list(out["id"]) == [0, 1, 2] and list(out["anchor"]) == [True, False, False]
    assert list(out["fasta"]) == ["d.fa", "b.fa", "c.fa"] and out["gff"].tolist()[1] == "b.gff"
    assert list(samples["id"]) == [0, 1, 2, 3]  # the source's table is not touched
