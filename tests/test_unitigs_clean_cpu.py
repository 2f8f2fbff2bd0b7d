"""CPU: the model of k_unitig_clean (tests/unitigs_clean_ref.py) held to a brute force over strings on seeded random graphs, the
rule's invariants on the same graphs, the crafted cases held to their promises, and the `novel` subcommand's new flags: what it
refuses before any work, the five statistic lines, and stdout without --clean as it was."""
import numpy as np
import pytest

from tests import unitigs_clean_ref as CR
from tests import unitigs_ref as UR

SEEDS = range(360)


@pytest.fixture(scope="module")
def cleaned():
    """[(seed, k, nodes, T, B, Rm, survivors, stats, every round's dropped keys)] of the random graphs — computed once"""
    out = []
    for seed in SEEDS:
        k, nodes, T, B, Rm = CR.random_graph(seed)
        trace = []
        left, st = CR.clean(nodes, k, T, B, Rm, CR.ROUNDS, trace=trace)
        out.append((seed, k, nodes, T, B, Rm, left, st, trace))
    return out


def test_the_model_equals_the_brute_force_on_random_graphs(cleaned):
    tips = bubbles = second = 0
    for seed, k, nodes, T, B, Rm, left, st, _ in cleaned:
        assert min(nodes.values()) <= 3 or max(nodes.values()) >= 10
        want, wst = CR.brute_clean(UR.strings_of(nodes, k), T, B, Rm, CR.ROUNDS)
        assert UR.strings_of(left, k) == want and st == wst, (seed, st, wst)
        tips += st["clipped_tips"] > 0
        bubbles += st["popped_bubbles"] > 0
        second += st["clean_rounds"] >= 2
    assert tips >= 20 and bubbles >= 20 and second >= 5, (tips, bubbles, second)


def test_the_rule_reads_the_same_from_either_end(cleaned):
    """a bubble is decided alike on U and on its reverse complement: the model walks from p, this walks from rc(q)"""
    for seed, k, nodes, T, B, Rm, _, _, _ in cleaned[:120]:
        for path, circular in UR.unitig_paths(nodes, k):
            if not circular:
                assert CR.is_bubble(path, nodes, k, B, Rm) == CR.is_bubble(CR.flip(path, k), nodes, k, B, Rm), (seed, path)


def test_invariants(cleaned):
    for seed, k, nodes, T, B, Rm, left, st, trace in cleaned:
        assert set(left) <= set(nodes) and all(left[x] == nodes[x] for x in left), seed
        assert len(nodes) - len(left) == st["clipped_kmers"] + st["popped_kmers"] == sum(len(d) for d in trace), seed
        assert st["clean_rounds"] == len(trace) <= CR.ROUNDS
        g = dict(nodes)
        for drop in trace:
            for path, circular in UR.unitig_paths(g, k):
                sides = [CR.right_side(path, g, k)[0], CR.right_side(CR.flip(path, k), g, k)[0]]
                if circular or sides == ["dead", "dead"]:  # no isolated unitig, and no circle, is ever dropped
                    assert not drop & set(UR.canon(w, k) for w in path), (seed, path)
                # at every fork that had a non-empty S, the deepest branch survives the round
                for P in (path, CR.flip(path, k)):
                    kind, v = CR.right_side(P, g, k)
                    if kind == "att" and UR.canon(P[-1], k) in drop and CR.is_tip(path, g, k, T, Rm):
                        S = [s for s in CR.preds(v, g, k) if s != P[-1]]
                        if S and CR.right_side(CR.flip(P, k), g, k)[0] == "dead":
                            deepest = max(g[UR.canon(s, k)] for s in S)
                            assert any(g[UR.canon(s, k)] == deepest and UR.canon(s, k) not in drop for s in S), (seed, P)
            g = {x: d for x, d in g.items() if x not in drop}
        assert g == left
        # a cleaned graph run again to exhaustion drops nothing
        if st["clean_rounds"] < CR.ROUNDS:
            assert CR.clean_round(left, k, T, B, Rm)[0] == set(), seed
        else:
            end, _ = CR.clean(left, k, T, B, Rm, 64)
            assert CR.clean_round(end, k, T, B, Rm)[0] == set(), seed


@pytest.mark.parametrize("k", CR.KS)
def test_the_crafted_cases_keep_their_promises(k):
    table, sets, promises = CR.crafted(k)
    raw = CR.crafted_nodes(k)
    left, st, _, _, U = CR.crafted_model(k)
    want, wst = CR.brute_clean(UR.strings_of(raw, k), CR.default_kmers(k), CR.default_kmers(k))
    assert UR.strings_of(left, k) == want and st == wst
    assert UR.brute_unitigs(want) == U
    assert 2 ** 11 <= len(raw) <= 2 ** 15 or k < CR.EXACT_FROM_K
    if k < CR.EXACT_FROM_K:
        return
    rawU = UR.unitigs(raw, k)
    linear = {seq for seq, _, _, c in U if not c}
    one_round = CR.clean(raw, k, rounds=1)[0]
    U1 = {seq for seq, _, _, c in UR.unitigs(one_round, k) if not c}
    seen = set()
    for case, kind, what in promises:
        seen.add(case)
        if kind == "one":
            assert what in linear and what not in {seq for seq, _, _, _ in rawU}, case
            if case == "tip_on_arm":
                assert what not in U1, case  # (open at rounds = 1)
        elif kind == "stays":
            assert what and all(x in left for x in what), case
        elif kind == "gone":
            assert what and all(x in raw and x not in left for x in what), case
        else:
            assert any(c and n == what for _, n, _, c in U) and not any(c and n == what for _, n, _, c in rawU), case
    assert seen == {"tip", "tip_long", "tip_ratio", "two_ends", "held_sibling", "isolated", "snp", "even", "indel", "arm_long", "tip_on_arm",
                    "circle", "odd_ends"}
    assert st["clean_rounds"] == 2 and CR.clean(raw, k, rounds=1)[1]["clean_rounds"] == 1
    # every case stands on both strands: four tips and three bubbles each
    assert st["clipped_tips"] >= 8 and st["popped_bubbles"] == 6


# ---------------------------------------------------------------------------
# the subcommand
# ---------------------------------------------------------------------------
def test_clean_flags_are_refused_before_any_work(tmp_path, capsys):
    from panagram_amd.__main__ import main
    fq = tmp_path / "s.fq"
    fq.write_text("@r\nACGT\n+\nIIII\n")
    u = ["--unitigs", str(tmp_path / "u.fa")]
    base = ["novel", str(tmp_path), str(fq)]
    for argv, what in ((base + ["--clean"], "--clean needs --unitigs"),
                       (base + ["--tip-kmers", "5"], "--tip-kmers needs --clean"),
                       (base + u + ["--bubble-kmers", "5"], "--bubble-kmers needs --clean"),
                       (base + u + ["--clean-ratio", "0.2"], "--clean-ratio needs --clean"),
                       (base + u + ["--clean-rounds", "2"], "--clean-rounds needs --clean"),
                       (base + ["--clean", "--clean-rounds", "2"], "--clean needs --unitigs"),
                       (base + u + ["--clean", "--clean-ratio", "0"], "--clean-ratio is above 0 and below 1"),
                       (base + u + ["--clean", "--clean-ratio", "1"], "--clean-ratio is above 0 and below 1"),
                       (base + u + ["--clean", "--clean-ratio", "-0.5"], "--clean-ratio is above 0 and below 1"),
                       (base + u + ["--clean", "--clean-ratio", "nan"], "--clean-ratio is above 0 and below 1"),
                       (base + u + ["--clean", "--tip-kmers", "0"], "1 to 1024"),
                       (base + u + ["--clean", "--bubble-kmers", "1025"], "1 to 1024"),
                       (base + u + ["--clean", "--clean-rounds", "65"], "0 to 64")):
        with pytest.raises(SystemExit) as ei:
            main(argv)
        assert ei.value.code == 2
        assert what in capsys.readouterr().err, argv
    assert not (tmp_path / "u.fa").exists()


class FakeIndex:
    """stands in for index.Index behind the subcommand: records what ``novel`` was asked and answers with hand-made frames"""
    calls = []

    def __init__(self, path, mode="r", device=0):
        self.genome_names = []

    def novel(self, samples, min_count, batch_bytes, **kw):
        from panagram_amd import novel as nov
        FakeIndex.calls.append(kw)
        counts = {"nkeys": 7, "solid": 5, "solid_windows": 11, "depth_hist": np.arange(64, dtype=np.uint64)}
        st = nov.stats(counts, 2, 100, 60, 3, 300, None)
        frame = nov.unitigs_frame([0, 7], [3, 2], [9, 4], [0, 0], np.frombuffer(b"ACGTACGCCGTAA", np.uint8), 5)
        out = (st, nov.spectrum_frame(counts["depth_hist"]), None, None)
        if kw.get("unitigs"):
            out += (frame,)
        if kw.get("clean") is not None:
            out += (dict(zip(nov.CLEAN_STAT_NAMES, (4, 40, 3, 33, 2))),)
        return out

    def close(self):
        pass


def test_the_stat_lines_and_stdout_without_clean(tmp_path, capsys, monkeypatch):
    from panagram_amd import index as pidx, novel as nov
    from panagram_amd.__main__ import main
    monkeypatch.setattr(pidx, "Index", FakeIndex)
    fq = tmp_path / "s.fq"
    fq.write_text("@r\nACGT\n+\nIIII\n")
    base = ["novel", str(tmp_path), str(fq)]
    FakeIndex.calls.clear()
    assert main(base) == 0
    plain = capsys.readouterr().out
    assert main(base + ["--unitigs", str(tmp_path / "u.fa")]) == 0
    with_unitigs = capsys.readouterr().out
    assert main(base + ["--unitigs", str(tmp_path / "c.fa"), "--clean", "--tip-kmers", "9", "--clean-ratio", "0.1"]) == 0
    with_clean = capsys.readouterr().out
    assert "clean" not in plain and "clipped" not in with_unitigs and with_unitigs.startswith(plain)
    assert with_unitigs == plain + "".join(x + "\n" for x in ["unitigs\t2", "unitig_bases\t13", "unitig_n50\t7", "longest_unitig\t7", "circular_unitigs\t0"])
    assert with_clean == with_unitigs + "clipped_tips\t4\nclipped_kmers\t40\npopped_bubbles\t3\npopped_kmers\t33\nclean_rounds\t2\n"
    assert nov.CLEAN_STAT_NAMES == CR.STAT_NAMES
    assert [c.get("clean") for c in FakeIndex.calls] == [None, None, {"tip_kmers": 9, "bubble_kmers": None, "ratio": 0.1, "rounds": None}]
    assert (tmp_path / "c.fa").read_text() == (tmp_path / "u.fa").read_text()


def test_clean_options():
    from panagram_amd import novel as nov
    assert nov.clean_options(21) == {"tip_kmers": 42, "bubble_kmers": 42, "ratio": 0.25, "rounds": 4}
    assert nov.clean_options(31, 5, 1024, 0.999, 0) == {"tip_kmers": 5, "bubble_kmers": 1024, "ratio": 0.999, "rounds": 0}
    for bad in (dict(tip_kmers=0), dict(bubble_kmers=1025), dict(ratio=0.0), dict(ratio=1.0), dict(ratio=0.0001), dict(ratio=0.9996), dict(rounds=-1),
                dict(rounds=65)):
        with pytest.raises(ValueError):
            nov.clean_options(21, **bad)
