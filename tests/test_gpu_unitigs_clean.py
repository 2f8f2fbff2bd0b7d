"""GPU: engine.NovelTable.clean (pg_unitigs.hip: k_unitig_clean, and k_unitig_links / k_unitig_links_emit / k_unitig_walk over the
drop plane) against the model (tests/unitigs_clean_ref.py), exactly: the statistics, the surviving keys and their link bytes, the
unitigs of the cleaned graph as a set, with the partition and maximality checks on the GPU's output alone; at k = 6, 21, 31, 32 on
the crafted cases (a few thousand keys, the table grown from 16 keys) and on about 40 seeded random graphs at k = 3 to 9; the
capacity protocol behind a clean; the raw graph back after rounds = 0, another min_count and an add; parameters out of range."""
import ctypes as C

import numpy as np
import pytest

from tests import novel_ref as NR
from tests import unitigs_clean_ref as CR
from tests import unitigs_ref as UR

pytestmark = pytest.mark.gpu

POISON = 0xA5
MC = CR.MIN_COUNT


def crafted_table(ctx, k):
    """(pan table, novel table) with both sets of the crafted sample added, the novel table grown from 16 keys"""
    from panagram_amd import engine
    table, sets, _ = CR.crafted(k)
    tbl = NR.pan_table(ctx, k, 8, table)
    nt = engine.NovelTable(tbl, capacity_keys=16)
    for s in sets:
        ss = engine.SeqSet.from_host(ctx, s)
        try:
            nt.add(ss)
        finally:
            ss.close()
    st = nt.stats()
    assert st["grown"] >= 2 and 2 ** 12 <= st["nslots"] <= 2 ** 16
    return tbl, nt


def same_graph(nt, k, mc, nodes, tag):
    """links() and unitigs() of the handle are those of the graph ``nodes``"""
    lk, lb = UR.links(nodes, k)
    keys, links = nt.links(mc)
    assert keys.tolist() == lk.tolist(), (tag, len(keys), len(lk))
    bad = np.flatnonzero(links != lb)
    assert len(bad) == 0, (tag, len(bad), keys[bad[:5]].tolist(), links[bad[:5]].tolist(), lb[bad[:5]].tolist())
    arrays = nt.unitigs(mc)
    got = UR.unpack(arrays, k)
    want = UR.unitigs(nodes, k)
    n = arrays["kmers"].astype(np.int64)
    assert arrays["offsets"].tolist() == (np.cumsum(n + k - 1) - (n + k - 1)).tolist() and len(arrays["bases"]) == int((n + k - 1).sum()), tag
    assert len(got) == len(set(got)) == len(want), (tag, len(got), len(want))
    missing, extra = want - set(got), set(got) - want
    assert not missing and not extra, (tag, sorted(missing)[:3], sorted(extra)[:3])
    UR.check_partition(set(got), nodes, k)
    UR.check_maximal(set(got), nodes, k)
    return arrays


@pytest.mark.parametrize("k", CR.KS)
def test_clean_equals_the_model_on_the_crafted_cases(ctx, k):
    from panagram_amd import engine
    tbl, nt = crafted_table(ctx, k)
    try:
        raw = CR.crafted_nodes(k)
        left, want, _, _, U = CR.crafted_model(k)
        before = nt.stats()
        st = nt.clean(MC)
        assert list(st) == CR.STAT_NAMES and st == want, (k, st, want)
        t = engine.novel_clean_last_timing()
        assert sorted(t) == ["clean_ms", "links_ms"] and t["links_ms"] > 0 and (t["clean_ms"] > 0 or k < CR.EXACT_FROM_K)
        same_graph(nt, k, MC, left, (k, "cleaned"))
        assert nt.stats() == before  # (the novel table is only read)
        if k >= CR.EXACT_FROM_K:
            assert st["clean_rounds"] == 2 and any(c and n == CR.CIRCLE for _, n, _, c in UR.unpack(nt.unitigs(MC), k))
        # one round: the tip on a bubble's arm leaves its bubble open
        left1, want1 = CR.clean(raw, k, rounds=1)
        assert nt.clean(MC, rounds=1) == want1
        same_graph(nt, k, MC, left1, (k, "one round"))
        # other limits and another ratio
        T, B, ratio = k, k + 3, 0.1
        left2, want2 = CR.clean(raw, k, T, B, 100, 3)
        assert nt.clean(MC, tip_kmers=T, bubble_kmers=B, ratio=ratio, rounds=3) == want2
        same_graph(nt, k, MC, left2, (k, "other limits"))
        # rounds = 0: the raw graph again
        assert nt.clean(MC, rounds=0) == dict(zip(CR.STAT_NAMES, [0] * 5))
        same_graph(nt, k, MC, raw, (k, "rounds = 0"))
        # another min_count: raw, whatever was cleaned before
        assert nt.clean(MC) == want
        same_graph(nt, k, 3, CR.crafted_nodes(k, 3), (k, "min_count 3"))
        same_graph(nt, k, MC, raw, (k, "back at min_count 2"))
    finally:
        nt.close()
        tbl.close()


def test_the_capacity_protocol_and_an_add_behind_a_clean(ctx):
    from panagram_amd import engine
    k = 21
    tbl, nt = crafted_table(ctx, k)
    try:
        left, want, lk, lb, U = CR.crafted_model(k)
        assert nt.clean(MC) == want
        full = same_graph(nt, k, MC, left, "full")
        nu, nb, nc = len(full["kmers"]), len(full["bases"]), int(full["circular"].sum())
        assert nu == len(U) and nc == sum(c for _, _, _, c in U) >= 2
        c0 = nt.unitigs(MC, cap_unitigs=0, cap_bases=0)
        assert (c0["nunitigs"], c0["nbases"], c0["ncircular"]) == (nu, nb, nc) and len(c0["bases"]) == 0
        k10, l10, n = nt.links(MC, cap=10)
        allk = dict(zip(lk.tolist(), lb.tolist()))
        assert n == len(left) and [allk[x] for x in k10.tolist()] == l10.tolist() and nt.links(MC, cap=0)[2] == n
        cu, cb = 40, int(full["offsets"][27]) + 5
        part = nt.unitigs(MC, cap_unitigs=cu, cap_bases=cb, fill=POISON)
        for f in ("offsets", "kmers", "depth_sum", "circular"):
            assert part[f].tolist() == full[f][:cu].tolist(), f
        assert part["bases"].tolist() == full["bases"][:cb].tolist()
        assert (part["nunitigs"], part["nbases"], part["ncircular"]) == (nu, nb, nc)
        tail = nt.unitigs(MC, cap_unitigs=nu - 1, cap_bases=nb - 1, fill=POISON)
        assert tail["circular"].tolist() == full["circular"][:nu - 1].tolist() and tail["bases"].tolist() == full["bases"][:nb - 1].tolist()
        again = nt.unitigs(MC)
        assert all(again[f].tolist() == full[f].tolist() for f in full)
        # an add: the raw graph of the larger sample, no stale plane
        table, sets, _ = CR.crafted(k)
        extra = [NR._rand(np.random.default_rng(5), 50 + k - 1)] * 2
        ss = engine.SeqSet.from_host(ctx, extra)
        try:
            nt.add(ss)
        finally:
            ss.close()
        _, _, nk, d = NR.novel_counts(table, sets + [extra], k)
        nodes = UR.nodes_of(nk, d, MC)
        assert len(nodes) == len(CR.crafted_nodes(k)) + 50
        same_graph(nt, k, MC, nodes, "after an add")
        left2, want2 = CR.clean(nodes, k)
        assert nt.clean(MC) == want2 and len(left2) == len(left) + 50
        same_graph(nt, k, MC, left2, "cleaned after an add")
        nt.clear()
        assert nt.clean(MC) == dict(zip(CR.STAT_NAMES, [0] * 5)) and len(nt.links(MC)[0]) == 0
        assert engine.novel_clean_last_timing() == {"links_ms": 0.0, "clean_ms": 0.0}
    finally:
        nt.close()
        tbl.close()


def test_random_graphs_loaded_as_tables(ctx):
    """every node a contig of its own, as often as it is deep; one pan table per k, the novel table cleared between graphs"""
    from panagram_amd import engine
    tables = {}
    try:
        done = dropped = 0
        for seed in range(42):
            k, nodes, T, B, Rm = CR.random_graph(seed)
            if k not in tables:
                tables[k] = engine.PanTable(ctx, k, 8)
            nt = engine.NovelTable(tables[k], capacity_keys=16)
            try:
                contigs = [UR.spell(x, k).encode() for x, d in sorted(nodes.items()) for _ in range(d)]
                ss = engine.SeqSet.from_host(ctx, contigs)
                try:
                    nt.add(ss)
                finally:
                    ss.close()
                same_graph(nt, k, 1, nodes, (seed, "raw"))
                left, want = CR.clean(nodes, k, T, B, Rm, CR.ROUNDS)
                got = nt.clean(1, tip_kmers=T, bubble_kmers=B, ratio=Rm / 1000.0, rounds=CR.ROUNDS)
                assert got == want, (seed, k, got, want)
                same_graph(nt, k, 1, left, (seed, "cleaned"))
                done += 1
                dropped += len(left) < len(nodes)
            finally:
                nt.close()
        assert done == 42 and dropped >= 15
    finally:
        for t in tables.values():
            t.close()


def test_parameters_out_of_range_are_refused(ctx):
    from panagram_amd import engine
    k = 21
    table, sets, _ = CR.crafted(k)
    tbl = NR.pan_table(ctx, k, 8, table)
    ss = engine.SeqSet.from_host(ctx, sets[0][:20])
    try:
        nt = engine.NovelTable(tbl, 16)
        nt.add(ss)
        lib = ctx._lib
        st = (C.c_uint64 * 5)()
        for args, what in (((1, 0, 5, 250, 4), b"tip_kmers"), ((1, 5, 0, 250, 4), b"bubble_kmers"), ((1, 1025, 5, 250, 4), b"tip_kmers"),
                           ((1, 5, 1025, 250, 4), b"bubble_kmers"), ((1, 5, 5, 0, 4), b"ratio_milli"), ((1, 5, 5, 1000, 4), b"ratio_milli"),
                           ((1, 5, 5, 250, 65), b"max_rounds"), ((0, 5, 5, 250, 4), b"min_count")):
            assert lib.pg_novel_clean(nt._h, *args, st) == -1 and what in lib.pg_last_error(), args
        assert lib.pg_novel_clean(nt._h, 1, 5, 5, 250, 4, None) == -1 and b"NULL" in lib.pg_last_error()
        assert lib.pg_novel_clean(None, 1, 5, 5, 250, 4, st) == -1
        assert lib.pg_novel_clean_last_timing(None) == -1
        assert lib.pg_novel_clean(nt._h, 1, 1, 1024, 999, 64, st) == 0 and lib.pg_novel_clean(nt._h, 1, 1024, 1, 1, 0, st) == 0
        for kw in (dict(tip_kmers=0), dict(bubble_kmers=1025), dict(ratio=0.0), dict(ratio=1.0), dict(rounds=65), dict(rounds=-1), dict(min_count=0)):
            with pytest.raises(ValueError):
                nt.clean(**kw)
        nt.close()
    finally:
        ss.close()
        tbl.close()
    tbl = engine.PanTable(ctx, 1, 8)  # k = 1 has no graph
    try:
        nt = engine.NovelTable(tbl, 16)
        with pytest.raises(engine.PanagramHipError) as ei:
            nt.clean(1, tip_kmers=2, bubble_kmers=2)
        assert ei.value.code == -1 and "k = 1" in str(ei.value)
        nt.close()
    finally:
        tbl.close()
