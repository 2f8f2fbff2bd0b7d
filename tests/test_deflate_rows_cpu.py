"""CPU: the model of the GPU BGZF encoder (tests/deflate_rows_ref.py) tied to zlib, and the crafted payloads of
tests/test_gpu_deflate_rows.py shown to hold what they promise — before any GPU is involved.  The model's tokens, written
with tests/deflate_craft.py, inflate to the payload; the size law gives the length of those very bytes; the ladder holds
every (run length, start residue) pair; the skewed counts need more than 15 bits; and four plausible mistakes of a
tokeniser change the size of at least one block of the inputs, so the exact-size assertion of the GPU tests can see them."""
import zlib

import numpy as np
import pytest

from tests import deflate_craft as dc
from tests import deflate_rows_ref as dr

ROWS = [1, 3, 38, 69, 255]
_cache = {}


def _payload(kind, row):
    key = (kind, row)
    if key not in _cache:
        if kind == "segments":
            _cache[key] = np.concatenate(dr.many_segments(8 * row)).reshape(-1)
        else:
            _cache[key] = {"ladder": dr.ladder, "edges": dr.edges, "skewed": dr.skewed}[kind](row)
    return _cache[key]


CASES = [(k, r) for r in ROWS for k in ("ladder", "edges")] + [("skewed", 1), ("segments", 1), ("segments", 3)]


@pytest.mark.parametrize("kind, row", CASES, ids=[f"{k}_{r}" for k, r in CASES])
def test_model_tokens_inflate_to_the_payload_and_the_size_law_gives_their_bytes(kind, row):
    p = _payload(kind, row)
    assert len(p) % row == 0
    ll = dc.huffman_lengths([int(f) for f in dr.file_hist(p, row)], 15)
    assert all(ll) and dc.kraft(ll) == 1 << 15
    for i, b in enumerate(dr.blocks_of(p)):
        toks = dr.tokens(b, row)
        h = dr.hist(b, row)
        lls, _ = dc.symbols(toks)
        assert np.array_equal(np.bincount(lls + [256], minlength=286), h), i
        assert sum(1 if isinstance(t, int) else t[1] for t in toks) == len(b), i
        body = dr.dynamic_body(toks, ll, row)
        ok, out, msg = dc.zlib_verdict(body)
        assert ok and out == b.tobytes(), (i, msg)
        hdr_ll, hdr_d, hdr_bits = dr.read_header(body)
        assert hdr_ll == ll and len(hdr_d) == dc.dist_symbol(row) + 1 and hdr_d[-1] == 1
        assert dr.sbytes(h, hdr_ll, row, hdr_d, hdr_bits) == len(body), i
        want, stored = dr.member_size(h, len(b), hdr_ll, row, hdr_d, hdr_bits)
        assert want == (18 + len(body) + 8 if not stored else 18 + 5 + len(b) + 8) and stored == (len(body) > dr.MAX_DYNAMIC)


def test_checker_passes_a_file_written_by_the_model_and_sees_a_wrong_one():
    """the assertions the GPU tests make (dr.check_file, dr.check_code), on a file the model wrote: dynamic blocks and a
    stored one; then one changed byte of a footer, of the index, and a block written under the tail-from-4 rule"""
    row = 3
    rnd = np.random.default_rng(1).integers(0, 256, dr.BLOCK, dtype=np.uint8)
    p = np.concatenate((dr.edges(row)[:2 * dr.BLOCK], rnd, dr.ladder(row)[:dr.BLOCK + 333]))
    gz, gzi = dr.model_file(p, row)
    import gzip
    assert gzip.decompress(gz) == p.tobytes()
    res = dr.check_file(gz, gzi, p, row)
    assert res["stored"] == [False, False, True, False, False] and res["sizes"] == res["want_sizes"]
    cost, hc, depth, lc = dr.check_code(res["ll_lens"], dr.file_hist(p, row))
    assert cost == lc and (hc == lc) == (depth <= 15)  # (the model writes package-merge lengths)
    mem = dr.members(gz)
    bad = bytearray(gz)
    bad[mem[1]["offset"] - 6] ^= 1  # CRC32 of block 0
    with pytest.raises(AssertionError, match="CRC32"):
        dr.check_file(bytes(bad), gzi, p, row)
    badi = bytearray(gzi)
    badi[8] ^= 1
    with pytest.raises(AssertionError, match="gzi"):
        dr.check_file(gz, bytes(badi), p, row)
    # block 3 (ladder) re-tokenised with tails of 3 as literals: still inflates, the exact size notices
    b = dr.blocks_of(p)[3]
    body = dr.dynamic_body(dr.tokens(b, row, tail_min=4), res["ll_lens"], row)
    assert dc.zlib_verdict(body)[1] == b.tobytes()
    other = gz[:mem[3]["offset"]] + dc.bgzf_member(body, b.tobytes()) + gz[mem[4]["offset"]:]
    assert gzip.decompress(other) == p.tobytes()
    with pytest.raises(AssertionError, match="blocks differ"):
        dr.check_file(other, None, p, row)


def test_skewed_counts_need_more_than_15_bits():
    p = dr.skewed()
    assert len(p) == 300 * 1023 and len(dr.blocks_of(p)) == 5
    total = sum(dr.hist(b, 1) for b in dr.blocks_of(p))
    assert total[257:].sum() == 0, "every byte of skewed is a literal"
    assert [int(total[v]) for v in dr.SKEW_VALUES] == [300 << j for j in range(10)]
    fh = dr.file_hist(p, 1)
    assert fh[256] == 5 and sorted(fh)[:275] == [1] * 275
    hc, depth = dr.huffman_cost(fh)
    assert depth >= 18
    lc = dr.limited_cost(fh, 15)
    assert hc < lc < dr.fixed_cost(fh)
    assert max(dc.huffman_lengths([int(f) for f in fh], 32)) == depth and dr.limited_cost(fh, 32) == hc


@pytest.mark.parametrize("row", ROWS + [2, 17, 68, 136])
def test_ladder_holds_every_run_length_at_every_residue(row):
    mask = dr.ladder_mask(row)
    got, s, e = dr.promised_runs(mask, row)
    assert got >= {(L, r) for L in dr.LADDER_LENGTHS for r in range(dr.CHUNK)}
    assert {L for L, _ in got} == set(dr.LADDER_LENGTHS) | set(range(3, 259))
    assert {1, 2, 3} <= set((s[1:] - e[:-1]).tolist()), "separators of 1, 2 and 3 bytes"
    assert 10 <= len(mask) / dr.BLOCK <= 14
    # the model sees the same runs: no run touches a block's first row, and the bytes follow the mask
    n = 13 if row == 2 else 300 if row == 38 else None
    p = dr.ladder(row, n)
    if n:
        assert not (p.reshape(-1, row)[:, -1] >> (n - 8 * (row - 1))).any(), "no bit past N"
    syms = np.zeros(286, np.int64)
    for i, b in enumerate(dr.blocks_of(p)):
        m = mask[i * dr.BLOCK:i * dr.BLOCK + len(b)]
        assert m[:row].all()
        eq = np.zeros(len(b), bool)
        eq[row:] = b[row:] == b[:-row]
        assert np.array_equal(eq, ~m), i
        syms += dr.hist(b, row)
    assert (syms[257:] > 0).all(), "every length symbol"
    assert set(range(3, 259)) <= set(np.concatenate([dr._structure(b, row)[2] for b in dr.blocks_of(p)]).tolist()), "every match length"


@pytest.mark.parametrize("row", ROWS)
def test_edges_hold_the_block_boundary_runs(row):
    p = dr.edges(row)
    blks = dr.blocks_of(p)
    assert len(blks) == 8
    for i in (1, 2, 3):  # one run over three whole blocks: each block is its first row and matches of 258 and a tail
        lit, ms, ml = dr._structure(blks[i], row)
        assert lit.sum() == row + ((dr.BLOCK - row) % 258 if (dr.BLOCK - row) % 258 < 3 else 0) and ms[0] == row
    lit, ms, ml = dr._structure(blks[4], row)
    assert ms[-1] + ml[-1] == dr.BLOCK and ml[-4:].sum() == 1000  # a run of 1000 ends on the block's last byte
    lit, ms, ml = dr._structure(blks[5], row)
    assert lit[:row].all() and ms[0] == row and ml[:3].sum() == 700  # a run of 700 starts at byte `row`
    lit, ms, ml = dr._structure(blks[6], row)
    assert lit.all() and len(ms) == 0  # no equal byte


MUTANTS = {"tail_from_4": dict(tail_min=4), "cut_at_257": dict(cut=257), "across_the_block_start": "before",
           "not_joined_across_68": dict(split=dr.CHUNK)}


@pytest.mark.parametrize("row", ROWS)
def test_inputs_can_see_a_wrong_tokeniser(row):
    """the per-block sizes under each mutated rule differ from the model's on some block of ladder or edges"""
    seen = {m: 0 for m in MUTANTS}
    for kind in ("ladder", "edges"):
        p = _payload(kind, row)
        ll = dc.huffman_lengths([int(f) for f in dr.file_hist(p, row)], 15)
        dl = [0] * dc.dist_symbol(row) + [1]
        for i, b in enumerate(dr.blocks_of(p)):
            true = dr.member_size(dr.hist(b, row), len(b), ll, row, dl, 700)
            for name, rule in MUTANTS.items():
                if rule == "before":
                    rule = dict(before=p[:i * dr.BLOCK])
                seen[name] += dr.member_size(dr.hist(b, row, **rule), len(b), ll, row, dl, 700) != true
    assert all(seen.values()), seen


def test_fit_block_reaches_every_size_around_the_threshold():
    """the threshold case's blocks, under the code the model expects for its background: sizes 65503..65518, one each"""
    base = dr.background_blocks(1)
    h = dr.hist(base, 1)
    assert h[257:].sum() == 0 and all(np.array_equal(dr.hist(b, 1), h) for b in dr.blocks_of(dr.background_blocks(4, seed=12)))
    fh = h * dr.SAMPLE + 1
    fh[256] = dr.SAMPLE
    ll = dc.huffman_lengths([int(f) for f in fh], 15)
    for t in range(65503, 65519):
        b = dr.fit_block(ll, [1], 800, t, t)
        assert len(b) == dr.BLOCK and dr.sbytes(dr.hist(b, 1), ll, 1, [1], 800) == t


def test_sample_blocks_and_members():
    assert dr.sample_blocks(5) == [0, 1, 2, 3, 4] and dr.sample_blocks(2048) == list(range(0, 2048, 4))
    assert len(dr.unsampled(513)) == 1 and len(dr.unsampled(600)) == 88
    body = dc.zlib_raw(b"abc" * 100)
    gz = dc.bgzf_member(body, b"abc" * 100, before=dc.subfield(b"X", b"Y", b"123")) + dc.EOF_MEMBER
    m = dr.members(gz)
    assert len(m) == 2 and m[0]["body"] == body and m[0]["isize"] == 300 and m[0]["crc"] == zlib.crc32(b"abc" * 100)
    assert m[1]["offset"] == m[0]["bsize"] + 1 and m[1]["isize"] == 0
