"""GPU: engine.NovelTable.links and .unitigs (pg_unitigs.hip: k_unitig_links, k_unitig_walk) against the model (tests/unitigs_ref.py),
exactly: the link byte of every solid key and the unitigs as a set of (canonical sequence, kmers, depth_sum, circular), at k = 6, 21,
31, 32 and at min_count 1, 2, 3 from ONE table that starts at 16 keys and has grown between the two adds; the partition invariant
on the GPU's output alone; the capacity protocol; a stale handle; the pan table only read; the timing's names; the empty cases.

As in tests/test_gpu_novel.py the crafted sample's own promises are asserted from k = 21 on (tests/test_unitigs_cpu.py); at k = 6
kernel and model still agree exactly."""
import numpy as np
import pytest

from tests import novel_ref as NR
from tests import unitigs_ref as UR

pytestmark = pytest.mark.gpu

THRESHOLDS = [1, 2, 3]
POISON = 0xA5


def crafted_table(ctx, k):
    """(pan table, novel table) with both sets of the crafted sample added, the novel table grown from 16 keys"""
    from panagram_amd import engine
    table, sets, _ = UR.crafted(k)
    first, both = UR.crafted_counts(k)
    tbl = NR.pan_table(ctx, k, 8, table)
    nt = engine.NovelTable(tbl, capacity_keys=16)
    for i, s in enumerate(sets):
        ss = engine.SeqSet.from_host(ctx, s)
        try:
            w, h, new = nt.add(ss)
        finally:
            ss.close()
        ref = first if i == 0 else (both[0] - first[0], both[1] - first[1], len(both[2]) - len(first[2]))
        assert (w, h, new) == (ref[0], ref[1], len(ref[2]) if i == 0 else ref[2]), (k, i)
    assert nt.stats()["grown"] >= 2
    return tbl, nt


def same_unitigs(arrays, k, min_count, tag):
    nodes, _, _, want = UR.crafted_model(k, min_count)
    assert arrays["offsets"].dtype == np.uint64 and arrays["kmers"].dtype == np.uint32 and arrays["depth_sum"].dtype == np.uint64
    assert arrays["circular"].dtype == np.uint8 and arrays["bases"].dtype == np.uint8
    got = UR.unpack(arrays, k)
    n = arrays["kmers"].astype(np.int64)
    # the offsets: the unitigs' bases back to back, nothing between them and nothing behind them
    assert arrays["offsets"].tolist() == (np.cumsum(n + k - 1) - (n + k - 1)).tolist() and len(arrays["bases"]) == int((n + k - 1).sum()), tag
    assert set(bytes(arrays["bases"])) <= set(b"ACGT"), tag
    assert len(got) == len(set(got)) == len(want), (tag, len(got), len(want))
    missing, extra = want - set(got), set(got) - want
    assert not missing and not extra, (tag, sorted(missing)[:3], sorted(extra)[:3])
    # on the GPU's output alone: every node in exactly one unitig, no compactable edge between two, a circle from its smallest key
    UR.check_partition(set(got), nodes, k)
    UR.check_maximal(set(got), nodes, k)
    assert not arrays["circular"][:-int(arrays["circular"].sum()) or None].any()  # (the circular ones stand behind the linear ones)
    return got


@pytest.mark.parametrize("k", UR.KS)
def test_links_and_unitigs_equal_the_model(ctx, k):
    from panagram_amd import engine
    tbl, nt = crafted_table(ctx, k)
    try:
        pan_before, novel_before = tbl.stats(), nt.stats()
        for mc in THRESHOLDS:
            nodes, lk, lb, want = UR.crafted_model(k, mc)
            keys, links = nt.links(mc)
            assert keys.dtype == np.uint64 and links.dtype == np.uint8 and keys.tolist() == lk.tolist(), (k, mc)
            bad = np.flatnonzero(links != lb)
            assert len(bad) == 0, (k, mc, len(bad), keys[bad[:5]].tolist(), links[bad[:5]].tolist(), lb[bad[:5]].tolist())
            t = engine.novel_unitigs_last_timing()
            assert sorted(t) == ["circular_ms", "links_ms", "walk_ms"] and t["links_ms"] > 0 and t["walk_ms"] == 0 and t["circular_ms"] == 0
            same_unitigs(nt.unitigs(mc), k, mc, (k, mc))
            t = engine.novel_unitigs_last_timing()
            assert t["links_ms"] > 0 and t["walk_ms"] > 0 and (t["circular_ms"] > 0) == any(c for _, _, _, c in want), (k, mc, t)
        assert tbl.stats() == pan_before and nt.stats() == novel_before  # (the pan table and the novel table are only read)
        if k >= UR.EXACT_FROM_K:
            by_seq = {seq: (n, ds, c) for seq, n, ds, c in UR.unpack(nt.unitigs(UR.MIN_COUNT), k)}
            assert by_seq[UR.crafted(k)[2]["long"]][0] == UR.LONG_KMERS
            assert sorted(n for n, _, c in by_seq.values() if c) == [3, 11, UR.CIRCLE]
    finally:
        nt.close()
        tbl.close()


def test_the_capacity_protocol(ctx):
    from panagram_amd import engine
    k, mc = 21, UR.MIN_COUNT
    tbl, nt = crafted_table(ctx, k)
    try:
        full = nt.unitigs(mc)
        got = same_unitigs(full, k, mc, "full")
        nu, nb, nc = len(full["kmers"]), len(full["bases"]), int(full["circular"].sum())
        assert nc == 3 and nu > 3000
        # counted only; the link keys' protocol is pg_novel_keys'
        c0 = nt.unitigs(mc, cap_unitigs=0, cap_bases=0)
        assert (c0["nunitigs"], c0["nbases"], c0["ncircular"]) == (nu, nb, nc) and len(c0["bases"]) == 0
        k10, l10, n = nt.links(mc, cap=10)
        allk = dict(zip(*(x.tolist() for x in nt.links(mc))))
        assert n == len(allk) and [allk[x] for x in k10.tolist()] == l10.tolist() and nt.links(mc, cap=0)[2] == n
        # caps below the totals: everything past them stays as it was — a unitig's bases may be cut
        cu, cb = 100, int(full["offsets"][57]) + 5
        part = nt.unitigs(mc, cap_unitigs=cu + 7, cap_bases=cb + 9, fill=POISON)
        for f in ("offsets", "kmers", "depth_sum", "circular"):
            assert part[f][:cu + 7].tolist() == full[f][:cu + 7].tolist(), f
        assert part["bases"].tolist() == full["bases"][:cb + 9].tolist()
        lib = ctx._lib
        import ctypes as C
        arrs = {f: np.full((cu + 7) * full[f].itemsize, POISON, np.uint8) for f in ("offsets", "kmers", "depth_sum", "circular")}
        bases = np.full(cb + 9, POISON, np.uint8)
        out = [C.c_uint64() for _ in range(3)]
        rc = lib.pg_novel_unitigs(nt._h, mc, cu, cb, *[a.ctypes.data_as(C.c_void_p) for a in arrs.values()], bases.ctypes.data_as(C.c_void_p),
                                  *[C.byref(x) for x in out])
        assert rc == 0 and [int(x.value) for x in out] == [nu, nb, nc]
        for f, a in arrs.items():
            a = a.view(full[f].dtype)
            assert a[:cu].tolist() == full[f][:cu].tolist() and (a[cu:].view(np.uint8) == POISON).all(), f
        assert bases[:cb].tolist() == full["bases"][:cb].tolist() and (bases[cb:] == POISON).all()
        # caps that reach into the circular ones, which stand last
        tail = nt.unitigs(mc, cap_unitigs=nu - 1, cap_bases=nb - 1, fill=POISON)
        assert tail["circular"].tolist() == full["circular"][:nu - 1].tolist() and tail["bases"].tolist() == full["bases"][:nb - 1].tolist()
        # the same answer on a second call, in the same order
        again = nt.unitigs(mc)
        assert all(again[f].tolist() == full[f].tolist() for f in full)
        # an add between the counting call and the filling call: no stale plane is served
        table, sets, _ = UR.crafted(k)
        assert nt.unitigs(mc, cap_unitigs=0, cap_bases=0)["nunitigs"] == nu
        extra = [NR._rand(np.random.default_rng(5), 50 + k - 1)] * 2 + [sets[0][0]]  # a new unitig of 50 k-mers; the first piece deepened
        ss = engine.SeqSet.from_host(ctx, extra)
        try:
            nt.add(ss)
        finally:
            ss.close()
        _, _, nk, d = NR.novel_counts(table, sets + [extra], k)
        nodes = UR.nodes_of(nk, d, mc)
        after = nt.unitigs(mc)
        assert set(UR.unpack(after, k)) == UR.unitigs(nodes, k) and len(after["kmers"]) == nu + 1
        lk, lb = nt.links(mc)
        assert (lk.tolist(), lb.tolist()) == tuple(x.tolist() for x in UR.links(nodes, k))
        # cleared and added again
        nt.clear()
        empty = nt.unitigs(mc)
        assert all(len(empty[f]) == 0 for f in empty) and len(nt.links(mc)[0]) == 0
        for s in sets:
            ss = engine.SeqSet.from_host(ctx, s)
            try:
                nt.add(ss)
            finally:
                ss.close()
        assert set(UR.unpack(nt.unitigs(mc), k)) == set(got)
    finally:
        nt.close()
        tbl.close()


def test_a_stale_handle_and_the_arguments_are_refused(ctx):
    from panagram_amd import engine
    k = 21
    table, sets, _ = UR.crafted(k)
    tbl = engine.PanTable(ctx, k, 8)
    ss = engine.SeqSet.from_host(ctx, sets[0][:50])
    try:
        NR.load(tbl, table[:-100], NR.masks(8, len(table))[:-100])
        nt = engine.NovelTable(tbl, 16)
        nt.add(ss)
        assert len(nt.unitigs(1)["kmers"]) > 0
        for bad in (0, 2 ** 32):
            with pytest.raises(ValueError, match="min_count"):
                nt.links(bad)
            with pytest.raises(ValueError, match="min_count"):
                nt.unitigs(bad)
        lib = ctx._lib
        import ctypes as C
        n3 = [C.c_uint64() for _ in range(3)]
        assert lib.pg_novel_unitigs(nt._h, 0, 0, 0, None, None, None, None, None, *[C.byref(x) for x in n3]) == -1 and b"min_count" in lib.pg_last_error()
        assert lib.pg_novel_links(nt._h, 0, 0, None, None, C.byref(n3[0])) == -1 and b"min_count" in lib.pg_last_error()
        assert lib.pg_novel_unitigs(nt._h, 1, 0, 0, None, None, None, None, None, None, None, None) == -1 and b"NULL" in lib.pg_last_error()
        assert lib.pg_novel_unitigs(nt._h, 1, 5, 0, None, None, None, None, None, *[C.byref(x) for x in n3]) == -1 and b"NULL" in lib.pg_last_error()
        assert lib.pg_novel_links(nt._h, 1, 5, None, None, C.byref(n3[0])) == -1 and b"NULL" in lib.pg_last_error()
        assert lib.pg_novel_unitigs_last_timing(None) == -1
        NR.load(tbl, table[-100:], NR.masks(8, len(table))[-100:])  # new keys behind the handle
        for call in (lambda: nt.links(1), lambda: nt.unitigs(1), lambda: nt.keys(1)):
            with pytest.raises(engine.PanagramHipError) as ei:
                call()
            assert ei.value.code == -1 and "changed behind the novel table" in str(ei.value)
        nt.close()
    finally:
        ss.close()
        tbl.close()
    tbl = engine.PanTable(ctx, 1, 8)  # k = 1 has no graph
    try:
        nt = engine.NovelTable(tbl, 16)
        for call in (lambda: nt.links(1), lambda: nt.unitigs(1)):
            with pytest.raises(engine.PanagramHipError) as ei:
                call()
            assert ei.value.code == -1 and "k = 1" in str(ei.value)
        nt.close()
    finally:
        tbl.close()


def test_an_empty_table_and_a_table_without_a_solid_key(ctx):
    from panagram_amd import engine
    k = 21
    table, sets, _ = UR.crafted(k)
    tbl = NR.pan_table(ctx, k, 8, table)
    try:
        nt = engine.NovelTable(tbl, 16)
        for mc in (1, 2):
            u = nt.unitigs(mc, cap_unitigs=4, cap_bases=4, fill=POISON)
            assert (u["nunitigs"], u["nbases"], u["ncircular"]) == (0, 0, 0) and (u["bases"] == POISON).all() and (u["kmers"].view(np.uint8) == POISON).all()
            assert nt.links(mc, cap=4)[2] == 0 and len(nt.unitigs(mc)["kmers"]) == 0
        assert engine.novel_unitigs_last_timing() == {"links_ms": 0.0, "walk_ms": 0.0, "circular_ms": 0.0}  # (nothing was launched)
        ss = engine.SeqSet.from_host(ctx, sets[0][:40])  # every k-mer once
        try:
            nt.add(ss)
        finally:
            ss.close()
        assert nt.result(1)["solid"] > 0 and nt.result(1000)["solid"] == 0
        u = nt.unitigs(1000, cap_unitigs=4, cap_bases=4, fill=POISON)
        assert (u["nunitigs"], u["nbases"], u["ncircular"]) == (0, 0, 0) and (u["bases"] == POISON).all()
        assert nt.links(1000, cap=4)[2] == 0
        assert engine.novel_unitigs_last_timing() == {"links_ms": 0.0, "walk_ms": 0.0, "circular_ms": 0.0}
        assert len(nt.unitigs(1)["kmers"]) > 0
        nt.close()
    finally:
        tbl.close()


def test_the_times_are_the_handles_own(ctx):
    """two novel tables used in turn in one thread: the times read behind a call are those of that call's table"""
    from panagram_amd import engine
    k = 21
    table, sets, _ = UR.crafted(k)
    tbl = NR.pan_table(ctx, k, 8, table)
    ss = engine.SeqSet.from_host(ctx, sets[0][:40])
    try:
        one, two = engine.NovelTable(tbl, 16), engine.NovelTable(tbl, 16)
        one.add(ss)
        two.add(ss)
        one.links(1)
        t1 = engine.novel_unitigs_last_timing()
        assert t1["links_ms"] > 0 and t1["walk_ms"] == 0
        two.unitigs(1)
        t2 = engine.novel_unitigs_last_timing()
        assert t2["links_ms"] > 0 and t2["walk_ms"] > 0
        one.links(1)  # (its planes are kept: nothing is added to its times, and nothing of the other table's shows)
        assert engine.novel_unitigs_last_timing() == t1
        two.links(1)
        assert engine.novel_unitigs_last_timing() == t2
        one.close()
        two.close()
    finally:
        ss.close()
        tbl.close()
