"""CPU: tests/fastq_craft.py — its byte-by-byte model (``walk``) against the split-based one (place_ref.fastq_model,
fastq_malformed) on the existing texts and on every crafted one, and, from a survey of each text's own offsets, that every crafted
text holds the edge its family claims: the byte at the offset asked, the line classes its tiles start in, its length, its tile
count, the tiles behind the last complete record, and the thread of k_fastq_offsets that owns each broken line's tile.  This is
what keeps tests/test_gpu_fastq_edges.py honest: a text that misses its edge fails here."""
import gzip

import pytest

from panagram_amd import place as pl
from tests import fastq_craft as fc
from tests import place_ref as pr

T = fc.T
GOOD, BAD = fc.well_formed(), fc.malformed()
OLD = pr.fastq_texts()


def _family(cases, family):
    sel = {n: c for n, c in cases.items() if c.claim["family"] == family}
    assert sel, family
    return sel


def _agree(text, tag):
    """walk == the split-based models; its tuple"""
    joined, nreads, consumed, first_bad = fc.walk(text)
    assert (joined, nreads, consumed) == pr.fastq_model(text), tag
    bad = pr.fastq_malformed(text)
    if not bad:
        assert first_bad is None, tag
    else:
        lines = bytes(text).split(b"\n")
        kind = "header" if not lines[4 * bad[0]].startswith(b"@") else "separator"
        assert first_bad == (bad[0], kind), tag
    return joined, nreads, consumed, first_bad


def test_walk_on_hand_made_texts():
    assert fc.walk(b"") == (b"", 0, 0, None) and fc.walk(b"\n\n\n") == (b"", 0, 0, None)
    assert fc.walk(b"@a\nAC\n+\nII\n@b\nGT\r\n+\nII\n@c\nTT") == (b"ACNGT", 2, 23, None)
    assert fc.walk(b"@a\n\r\n+\nII\n@b\nG\rT\r\r\n+\n\n") == (b"NG\rT\r", 2, 22, None)
    assert fc.walk(b"\n\n\n\n") == (b"", 1, 4, (0, "header"))
    assert fc.walk(b"@\n\n\n\n") == (b"", 1, 5, (0, "separator"))
    assert fc.walk(b"@a\nA\n+\n@\nb\nC\n-\n+\n") == (b"ANC", 2, 17, (1, "header"))  # (the header's rule before the separator's)
    assert fc.walk(b"@a\nA\n+\n@\n@b\nC\n-\n+\nx\nG\n-\n") == (b"ANC", 2, 18, (1, "separator"))  # (the torn record is not looked at)
    assert fc.walk(b"@a\nA\n+\n@\n@b\nC\n-\n+")[:3] == (b"A", 1, 9) and fc.walk(b"@a\nA\n+\n@\n@b\nC\n-\n+")[3] is None
    assert fc.walk(bytearray(b"+a\nA\n+\nI\n"))[3] == (0, "header")


@pytest.mark.parametrize("name", sorted(OLD))
def test_walk_equals_the_split_model_on_the_existing_texts(name):
    assert _agree(OLD[name], name)[3] is None


def test_walk_equals_the_split_model_on_the_existing_malformed_texts():
    for name, (text, bad) in pr.fastq_malformed_texts().items():
        first = _agree(text, name)[3]
        assert first[0] == bad[0] and first[1] == ("separator" if name == "no_plus" else "header"), name


def test_the_survey_helpers_on_a_hand_made_text():
    text = b"@a\nAC\n+\nII\n" + b"@b\n" + b"G" * (T - 11 - 3) + b"\nx"
    assert len(text) == T + 2 and fc.ntiles(text) == 2 and fc.ntiles(text[:T]) == 1 and fc.ntiles(b"") == 0
    assert fc.line_starts(text).tolist() == [0, 3, 6, 8, 11, 14, T + 1] and fc.line_starts(text[:-1]).tolist()[-1] == 14
    assert fc.line_at(text, 0) == 0 and fc.line_at(text, 2) == 0 and fc.line_at(text, 3) == 1 and fc.line_at(text, T) == 5
    assert fc.tile_starts(text) == [(0, True), (5, False)] and fc.tile_starts(text[1:]) == [(0, True), (6, True)]
    assert fc.tile_of_line(text, 5) == 0 and fc.tile_of_line(text, 6) == 1
    assert [fc.per_thread(n) for n in (1, 255, 256, 257, 512, 513)] == [1, 1, 1, 2, 2, 3]
    assert fc.owner(257, 255) == 127 and fc.owner(257, 256) == 128 and fc.owner(513, 512) == 170 and fc.owner(256, 255) == 255
    assert fc.malformed_lines(text) == [] and fc.malformed_lines(b"a\n\n-\n\n\n\n\n\n@\n\n\n") == [0, 2, 4, 6]
    assert fc.broken(text, 0, 2) == b"xa\nAC\n-\nII\n" + text[11:] and fc.first_line_in_tile(text, 0, 0, last=True) == 4
    with pytest.raises(AssertionError):
        fc.broken(fc.broken(text, 2), 2)


def test_placed_puts_the_feature_where_asked():
    for eol in (fc.LF, fc.CRLF):
        for f in fc.FEATURES:
            if f.startswith("cr") and eol == fc.LF:
                with pytest.raises(ValueError):
                    fc.placed(f, T, eol)
                continue
            text, offs = fc.placed(f, T + 3, eol)
            assert offs[f] == T + 3 and set(offs) == {x for x in fc.FEATURES if eol == fc.CRLF or not x.startswith("cr")}
            assert 2 <= fc.ntiles(text) <= 3 and fc.walk(text)[1:] == (4, len(text), None)
    with pytest.raises(ValueError):
        fc.placed("first0", 5, record=0)
    with pytest.raises(ValueError):
        fc.placed("first1", 2)


def _check_features(name, case):
    """the bytes named in claim["offsets"] are what they are called, and the one asked lies at claim["offset"]"""
    text, c = case.text, case.claim
    offs, starts = c["offsets"], set(fc.line_starts(text).tolist())
    assert offs[c["feature"]] == c["offset"], name
    rec = {fc.line_at(text, o) >> 2 for o in offs.values()}
    assert len(rec) == 1, name  # (all of one record)
    for f, o in offs.items():
        line = int(f[-1])
        assert fc.line_at(text, o) & 3 == line, (name, f)
        if f.startswith("first"):
            assert o in starts, (name, f)
        elif f.startswith("lf"):
            assert text[o] == 0x0A, (name, f)
        else:
            assert text[o:o + 2] == b"\r\n", (name, f)
    return rec.pop()


def test_slide_holds_every_feature_at_the_tile_edge_and_the_lane_edge():
    cases = _family(GOOD, "slide")
    seen = set()
    for name, case in cases.items():
        text, c = case.text, case.claim
        joined, nreads, consumed, first_bad = _agree(text, name)
        assert first_bad is None and 2 <= fc.ntiles(text) <= 3, name
        rec = _check_features(name, case)
        if c.get("last"):
            assert rec == nreads - 1 and consumed < len(text), name
            if c["feature"] == "lf3":
                assert consumed == c["offset"] + 1, name
        else:
            assert 0 < rec < nreads - 1 and consumed == len(text), name
        if c.get("empty"):
            assert text[c["offset"] - 1:c["offset"] + 2] == b"\n\r\n" and b"NN" in joined + b"N", name
        seen.add((c["eol"], c["feature"], c["offset"], bool(c.get("last"))))
    for eol in (fc.LF, fc.CRLF):
        for off in fc.SLIDE_OFFSETS:
            for f in fc.FEATURES:
                if eol == fc.CRLF or not f.startswith("cr"):
                    assert (eol, f, off, False) in seen, (f, off)
            assert (eol, "lf3", off, True) in seen and (eol, "first3", off, True) in seen
    # a '\r' as the last byte of a tile / of a lane's 16, its line feed the first of the next: of a sequence line, of the quality
    # line that ends `consumed`, of an empty sequence line
    for name, last in (("slide_crlf_cr1_%d", False), ("slide_crlf_last_cr3_%d", True), ("slide_crlf_empty_seq_%d", False),
                       ("slide_crlf_last_empty_seq_%d", True)):
        for off in (T - 1, T + 15):
            text = cases[name % off].text
            assert text[off:off + 2] == b"\r\n" and (off + 1) % 16 == 0, name
            if last and "cr3" in name:
                assert fc.walk(text)[2] == off + 2


def test_phases_start_a_tile_in_every_line_class_at_a_line_start_and_mid_line():
    cases = _family(GOOD, "phases")
    assert {c.claim["eol"] for c in cases.values()} == {fc.LF, fc.CRLF}
    for name, case in cases.items():
        text = case.text
        joined, nreads, consumed, first_bad = _agree(text, name)
        assert first_bad is None and consumed == len(text) and fc.ntiles(text) >= 9, name
        assert (b"\r\n" in text) == (case.claim["eol"] == fc.CRLF) and text.count(b"\r") == (4 * nreads if b"\r" in text else 0)
        tiles = [(line & 3, at_start) for line, at_start in fc.tile_starts(text)]
        assert {k: tiles[k] for k in case.claim["want"]} == case.claim["want"], name
        assert set(tiles[1:9]) == {(c, s) for c in range(4) for s in (True, False)}, name


def test_lengths_are_exact():
    cases = _family(GOOD, "lengths")
    assert sorted((c.claim["nbytes"], c.claim["eol"]) for c in cases.values() if not c.claim["torn"]) == \
        sorted((n, e) for n in (T, 2 * T, T - 16, T + 16, 16, 15) for e in (fc.LF, fc.CRLF))
    for name, case in cases.items():
        text, c = case.text, case.claim
        joined, nreads, consumed, first_bad = _agree(text, name)
        assert len(text) == c["nbytes"] and first_bad is None and nreads >= 1, name
        if c["torn"]:
            assert len(text) == T and text.endswith(b"\r") and text[-2] in b"ACGTI", name
            assert consumed < len(text) and b"\r" not in joined and b"\n" not in text[consumed:][-50:], name
        else:
            assert consumed == len(text) and text.endswith(c["eol"]) and (c["eol"] == fc.CRLF) == (b"\r" in text), name
    assert {fc.line_at(cases[f"length_cr_last_line{n}"].text, T - 1) & 3 for n in (1, 3)} == {1, 3}


def test_torn_tails_put_whole_tiles_behind_the_last_complete_record():
    cases = _family(GOOD, "torn_tail")
    torn_in = set()
    for name, case in cases.items():
        text, c = case.text, case.claim
        joined, nreads, consumed, first_bad = _agree(text, name)
        assert nreads == c["nreads"] and first_bad is None and consumed < len(text), name
        tiles = fc.tile_starts(text)
        assert fc.ntiles(text) >= 4 and consumed > T, name  # (the complete records fill more than a tile)
        assert all(line >= 4 * nreads for line, _ in tiles[-2:]) and tiles[-2][0] == tiles[-1][0] == 4 * nreads + c["line"], name
        assert len(text) - int(fc.line_starts(text)[-1]) >= 3 * T and not text.endswith(b"\n"), name  # the unfinished line
        assert sum(line < 4 * nreads for line, _ in tiles) >= 2, name
        lines = text[consumed:].split(b"\n")
        hidden = not lines[0].startswith(b"@") or (len(lines) > 2 and not lines[2].startswith(b"+"))
        assert hidden == c["hidden"], name
        if hidden:
            assert not lines[0].startswith(b"@") and not lines[2].startswith(b"+"), name
        torn_in.add((c["line"], b"\r\n" in text))
    assert torn_in == {(line, crlf) for line in range(4) for crlf in (False, True)}


def test_tile_counts_are_exact():
    cases = _family(GOOD, "tile_counts")
    assert sorted(c.claim["ntiles"] for c in cases.values()) == [255, 256, 257, 512, 513]
    assert {c.claim["eol"] for c in cases.values()} == {fc.LF, fc.CRLF}
    for name, case in cases.items():
        text, c = case.text, case.claim
        joined, nreads, consumed, first_bad = _agree(text, name)
        assert -(-len(text) // T) == c["ntiles"] == fc.ntiles(text) and first_bad is None and consumed == len(text), name
        assert (c["eol"] == fc.CRLF) == (b"\r" in text) and 1 << 20 <= len(text) + T <= (2 << 20) + 3 * T, name
        assert 95 < len(joined) / nreads < 106, name  # records of about 100 bases
    assert len(cases["tiles_255"].text) % T == 0 and len(cases["tiles_256"].text) % T == 1  # a full last tile; one of one byte
    # per: 1, 1, 2, 2, 3; the last thread with tiles has one (257), all of its range (512, 513); threads without a tile
    own = {nt: [fc.owner(nt, t) for t in range(nt)] for nt in (255, 256, 257, 512, 513)}
    assert own[255][-1] == 254 and own[256][-1] == 255 and own[257][-2:] == [127, 128] and own[512][-1] == 255
    assert own[513][-3:] == [170, 170, 170] and own[513].count(170) == 3


def test_hidden_malformed_lines_lie_behind_the_last_complete_record():
    for name, case in _family(GOOD, "hidden").items():
        text, c = case.text, case.claim
        joined, nreads, consumed, first_bad = _agree(text, name)
        assert first_bad is None and nreads == c["nreads"] and consumed < len(text), name
        assert _check_features(name, case) == nreads, name  # (the record behind the last complete one)
        lines = text[consumed:].split(b"\n")
        assert len(lines) == 4 and not lines[0].startswith(b"@") and not lines[2].startswith(b"+"), name
        assert text[c["offset"]] in b"x-", name


def test_malformed_texts_break_the_line_they_claim():
    assert len(BAD) > 60
    placed_at, phase_tiles, threads = set(), set(), {}
    for name, case in BAD.items():
        text, c = case.text, case.claim
        joined, nreads, consumed, first_bad = _agree(text, name)
        assert first_bad == c["first"] and c["first"] == (c["first_line"] >> 2, fc.kind_of(c["first_line"])), name
        line = c["first_line"]
        at = int(fc.line_starts(text)[line])
        assert line < 4 * nreads and text[at] not in b"@+", name
        if "offset" in c:  # placed: the offending byte at the offset asked
            assert at == c["offset"] and _check_features(name, case) == line >> 2, name
            if c.get("empty"):
                assert at % T == 0 and at > 0, name
                assert text[at:at + 2] == b"\r\n" if b"\r" in text else text[at] == 0x0A, name  # a lone line end
            if c.get("last"):
                assert line >> 2 == nreads - 1 and consumed < len(text), name
            placed_at.add((fc.kind_of(line), at, b"\r" in text, line >> 2 == 0, bool(c.get("last")), bool(c.get("empty"))))
        else:  # one line of a larger text broken: the tile it lies in, the phase the tile starts in, the thread that owns it
            assert fc.tile_of_line(text, line) == c["tile"], name
            if "phase" in c:
                tl, at_start = fc.tile_starts(text)[c["tile"]]
                assert (tl & 3, at_start) == (c["phase"], c["at_start"]), name
                if at_start and c["phase"] in (0, 2):
                    assert at == c["tile"] * T, name
                phase_tiles.add((b"\r" in text, c["phase"], at_start, fc.kind_of(line)))
            if "thread" in c:
                nt = fc.ntiles(text)
                assert fc.owner(nt, c["tile"]) == c["thread"] and fc.per_thread(nt) > 1, name
                threads.setdefault(nt, set()).add(c["thread"])
                if "later" in c:
                    lline, ltile, lthread = c["later"]
                    lat = int(fc.line_starts(text)[lline])
                    assert lline > line and lline < 4 * nreads and text[lat] not in b"@+" and lat // T == ltile, name
                    assert fc.owner(nt, ltile) == lthread and fc.kind_of(lline) != fc.kind_of(line), name
                    assert (lthread == c["thread"]) == name.endswith("one_thread"), name
                    assert ltile != c["tile"], name
                    assert fc.malformed_lines(text) == [line, lline], name  # (the later line the only one of its kind)
                else:
                    assert fc.malformed_lines(text) == [line], name
    for crlf in (False, True):
        for kind in ("header", "separator"):
            for off in (T - 1, T, T + 15, T + 16):
                assert (kind, off, crlf, False, False, False) in placed_at and (kind, off, crlf, False, True, False) in placed_at
            assert (kind, T, crlf, False, False, True) in placed_at and (kind, 2 * T, crlf, False, False, True) in placed_at
        assert ("header", 0, crlf, True, False, False) in placed_at
        assert {("separator", off, crlf, True, False, False) for off in (T - 1, T, T + 16)} <= placed_at
        assert {(ph, s) for c, ph, s, _ in phase_tiles if c == crlf} == {(ph, s) for ph in range(4) for s in (True, False)}
        assert {k for c, _, _, k in phase_tiles if c == crlf} == {"header", "separator"}
    # tile 0, the last tile, the last tile of a thread's range and the first of the next thread's; a thread past the 128th
    for nt in (257, 513):
        per = fc.per_thread(nt)
        text = fc.tile_counts()[f"tiles_{nt}"].text
        assert fc.ntiles(text) == nt
        spot = {s: BAD[f"bad_tiles_{nt}_{s}"].claim for s in ("tile0", "last_tile", "range_end", "next_range")}
        assert spot["tile0"]["tile"] == 0 and spot["last_tile"]["tile"] == nt - 1 and spot["last_tile"]["thread"] >= 128
        assert spot["range_end"]["tile"] % per == per - 1 and spot["next_range"]["tile"] == spot["range_end"]["tile"] + 1
        assert spot["next_range"]["thread"] == spot["range_end"]["thread"] + 1
        assert {fc.kind_of(c["first_line"]) for c in spot.values()} == {"header", "separator"}
        assert len(threads[nt]) >= 6


def test_the_batch_text_tears_at_every_batch_size(tmp_path):
    """the streaming that tests/test_gpu_fastq_edges.py runs on the GPU, under ``walk``: every batch size reassembles the whole,
    and some batch holds no complete record"""
    whole = fc.batch_text()
    joined, nreads, consumed, first_bad = _agree(whole, "batch text")
    assert 35_000 < len(whole) < 45_000 and consumed == len(whole) and first_bad is None and whole.count(b"\r\n") == 4 * nreads
    reads = joined.split(b"N")
    assert max(map(len, reads)) > 3 * T and reads.count(b"") >= 5 and reads[0] == b"" and reads[-1] == b""
    plain, gz = str(tmp_path / "a.fq"), str(tmp_path / "a.fq.gz")
    open(plain, "wb").write(whole)
    with gzip.open(gz, "wb") as f:
        f.write(whole)
    for path, sizes in ((plain, fc.BATCH_SIZES), (gz, fc.BATCH_SIZES[:1])):
        for b in sizes:
            fb = pl.FastqBatches(path, b)
            parts, total, empty = [], 0, 0
            for buf in fb:
                j, n, used, bad = fc.walk(buf)
                assert bad is None
                if n:
                    parts.append(j)
                empty += n == 0
                total += n
                fb.advance(used)
            assert (b"N".join(parts), total) == (joined, nreads) and empty >= 1, b
