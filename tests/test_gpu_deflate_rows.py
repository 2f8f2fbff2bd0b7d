"""GPU: the BGZF encoder of pg_deflate.hip (write_bgzf(level=-2): k_df_sample_hist, k_df_build_code, k_row_deflate) on rows
PLANTED into a rows container (tests/rows_craft.py), held to the model of tests/deflate_rows_ref.py: run lengths against the
68-byte chunk of a thread and the steps of its mask, runs over block boundaries, row widths of 1 to 255 bytes, the 15-bit
limit of the code lengths, blocks the sample never saw, the stored-block threshold to the byte, hundreds of payload segments
with poisoned padding between them, and contig ranges.

For every file (dr.check_file, dr.check_code):
  (a) it inflates (zlib) to the planted payload          (b) every member's CRC32 / ISIZE; the 28-byte EOF block
  (c) the .gzi: count, offsets i * 65280, running sum of BSIZE + 1
  (d) one header for all dynamic blocks                  (e) 286 code lengths of 1..15 bits, Kraft sum exactly 1
  (f) EXACT SIZE: BSIZE + 1 of every block = the size law on the model's counts of that block under the file's own code
      lengths; stored exactly when the law says so
  (g) the code's cost on the file's counts: the Huffman optimum where that needs no more than 15 bits, else between
      package-merge and the fixed code, and monotone in the counts
tests/test_deflate_rows_cpu.py shows that the inputs hold what they promise and that (f) sees a wrong tokeniser."""
import gzip
import os

import numpy as np
import pytest

from tests import deflate_rows_ref as dr
from tests import rows_craft as rc

pytestmark = pytest.mark.gpu

K = 21


def _write(ctx, tmp_path, n, rows_per_contig, files, **geometry):
    """plant the contigs' rows (padding and slack poisoned), run the statistics, write one file per (step, first contig,
    number of contigs or None); returns [(gz bytes, gzi bytes, payload bytes)]"""
    row = rc.row_bytes(n)
    rows_per_contig = [np.ascontiguousarray(r, np.uint8).reshape(-1, row) for r in rows_per_contig]
    low = geometry.get("lowres_step", 100)
    res = rc.container(ctx, K, n, [len(r) for r in rows_per_contig], **geometry)
    out = []
    try:
        rc.plant(res, rows_per_contig, poison=dr.POISON)
        res.rows_epilogue()
        for i, (step, first, nc) in enumerate(files):
            gz, gzi = str(tmp_path / f"f{i}.gz"), str(tmp_path / f"f{i}.gzi")
            res.write_bgzf(step, gz, gzi, level=-2, first_contig=first, ncontigs=nc)
            last = len(rows_per_contig) if nc is None else first + nc
            payload = b"".join(r[::(1 if step == 1 else low)].tobytes() for r in rows_per_contig[first:last])
            out.append((open(gz, "rb").read(), open(gzi, "rb").read(), payload))
            os.remove(gz)
            os.remove(gzi)
    finally:
        res.close()
    return out


def _check(gz, gzi, payload, row, code=True, hists=None):
    assert gzip.decompress(gz) == payload
    res = dr.check_file(gz, gzi, payload, row, hists=hists)
    if code and res["ll_lens"] is not None:
        res["cost"] = dr.check_code(res["ll_lens"], dr.file_hist(payload, row, res["hists"]))
    return res


# ---------------------------------------------------------------------------
# run geometry, at every row width
# ---------------------------------------------------------------------------
GEOMETRY_N = [8 * w for w in (1, 2, 3, 4, 5, 8, 17, 38, 65, 67, 68, 69, 96, 97, 128, 136, 255)] + [13, 300]


@pytest.mark.parametrize("n", GEOMETRY_N)
def test_run_geometry_at_every_row_width(ctx, n, tmp_path):
    """ladder: runs of 1..5, 30..34, 62..70, 94..98, 134..138, 255..261, 515..519, 774..777 and 1032 equal bytes starting at
    every byte of a thread's 68-byte chunk, and every match length 3..258; edges: a run over three whole blocks, one that
    ends on a block's last byte, one that starts at byte `row`, a block without an equal byte.  N = 13 and 300: a last row
    byte with bits past N (clear)."""
    row = rc.row_bytes(n)
    for kind in (dr.ladder, dr.edges):
        p = kind(row, n)
        (gz, gzi, payload), = _write(ctx, tmp_path, n, [p], [(1, 0, None)])
        assert payload == p.tobytes()
        _check(gz, gzi, payload, row)


def test_rows_of_256_bytes_take_the_host_writer(ctx, tmp_path):
    """level=-2 on a width the GPU encoder does not take: still a valid file with the payload, (a) to (c)"""
    n, row = 2048, 256
    p = dr.edges(row)[:row * 700]
    (gz, gzi, payload), = _write(ctx, tmp_path, n, [p], [(1, 0, None)])
    assert payload == p.tobytes() and gzip.decompress(gz) == payload
    dr.check_file(gz, gzi, payload, row, modelled=False)


def test_forced_stored_blocks(ctx, tmp_path, monkeypatch):
    p = dr.ladder(3)
    monkeypatch.setenv("PG_DEFLATE_FORCE_STORED", "1")
    (gz, gzi, payload), = _write(ctx, tmp_path, 24, [p], [(1, 0, None)])
    monkeypatch.delenv("PG_DEFLATE_FORCE_STORED")
    res = _check(gz, gzi, payload, 3)
    assert all(res["stored"]) and len(res["stored"]) == len(dr.blocks_of(p))
    assert len(gz) == len(payload) + 31 * len(res["stored"]) + 28


# ---------------------------------------------------------------------------
# tail blocks
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("row", [1, 3, 69])
def test_tail_blocks(ctx, row, tmp_path):
    """single-contig files of T bytes: one and two rows, around the chunk of 68, a last dword of 1..3 bytes, around one block
    and exactly two"""
    want = [1, 2, 3, row - 1, row, row + 1, 2 * row, 67, 68, 69, 4 * 25 + 1, 4 * 25 + 2, 4 * 25 + 3, dr.BLOCK - 1, dr.BLOCK,
            dr.BLOCK + 1, 2 * dr.BLOCK]
    want += [m // row * row + d for m in (dr.BLOCK, 2 * dr.BLOCK) for d in (0, row)]  # (whole rows next to the blocks' ends)
    ts = sorted({t for t in want if t > 0 and t % row == 0})
    assert row in ts and 2 * row in ts
    rng = np.random.default_rng(row)
    mask = rng.random((2 * dr.BLOCK // row + 9) * row) < 0.2
    full = dr.from_mask(mask, row, 40 + row)
    for t in ts:
        p = full[row * (t % 7):][:t]
        (gz, gzi, payload), = _write(ctx, tmp_path, 8 * row, [p], [(1, 0, None)])
        assert payload == p.tobytes(), t
        res = _check(gz, gzi, payload, row)
        assert len(res["sizes"]) == (t + dr.BLOCK - 1) // dr.BLOCK, t


# ---------------------------------------------------------------------------
# payload segments and contig ranges
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("n", [8, 24])
def test_segments_and_ranges(ctx, n, tmp_path):
    """312 contigs — 300 of one row, then 2, 3, 5, 15, 16, 17, 100, 1, 4000, 1, 1 and 70001 rows — that continue one pattern, so
    runs and matches cross the segments' boundaries; the padding between the contigs holds 0xA5 and no row byte does; steps 1,
    100 and 7; all contigs, all but the first and last, one one-row contig, the last contig"""
    row = rc.row_bytes(n)
    rows = dr.many_segments(n)
    nc = len(rows)
    ranges = [(0, None), (1, nc - 2), (150, 1), (nc - 1, 1)]
    for geometry, steps in (({}, (1, 100)), (dict(lowres_step=7), (7,))):
        files = [(s, f, m) for s in steps for f, m in ranges]
        for (s, f, m), (gz, gzi, payload) in zip(files, _write(ctx, tmp_path, n, rows, files, **geometry)):
            tag = f"step {s} contigs {f}+{m}"
            assert dr.POISON not in payload and len(payload) > 0, tag
            if (f, m) == (150, 1):
                assert len(payload) == row, tag
            _check(gz, gzi, payload, row)
            assert dr.POISON not in gzip.decompress(gz), tag


# ---------------------------------------------------------------------------
# the 15-bit limit
# ---------------------------------------------------------------------------
def test_code_length_limit(ctx, tmp_path, capsys):
    """ten literals with counts 300 * 2^j over 275 symbols of count 1: the unlimited Huffman code is 19 bits deep, the Kraft
    repair of df_huff_from_sorted has to run.  The measured cost over package-merge is printed, not bounded."""
    p = dr.skewed()
    fh = dr.file_hist(p, 1)
    hc, depth = dr.huffman_cost(fh)
    assert depth >= 16
    (gz, gzi, payload), = _write(ctx, tmp_path, 8, [p], [(1, 0, None)])
    res = _check(gz, gzi, payload, 1)
    assert res["ll_lens"] is not None
    cost, hc2, depth2, lc = res["cost"]
    assert (hc2, depth2) == (hc, depth) and len(res["sizes"]) == 5
    assert max(res["ll_lens"]) == 15
    with capsys.disabled():
        print(f"\nlength-limited code: cost {cost} bits, package-merge {lc}, unlimited Huffman {hc} (depth {depth}), "
              f"fixed {dr.fixed_cost(fh)}: cost / limited_cost = {cost / lc:.6f}")


# ---------------------------------------------------------------------------
# 600 blocks: blocks the sample skips, and the stored-block threshold to the byte
# ---------------------------------------------------------------------------
NBLOCKS = 600
_big = {}


def _background():
    """the 600-block payload (row width 1) and the model's counts of its blocks, made once"""
    if not _big:
        p = dr.background_blocks(NBLOCKS)
        _big["payload"] = p
        _big["hists"] = {i: dr.hist(b, 1) for i, b in enumerate(dr.blocks_of(p))}
        _big["skip"] = dr.unsampled(NBLOCKS)
    return _big


def _special(p):
    """three blocks the sample skips: a block of the ladder, all 256 byte values, random bytes; returns their indices"""
    skip = _background()["skip"]
    at = [skip[0], skip[40], skip[-1]]
    p[at[0] * dr.BLOCK:(at[0] + 1) * dr.BLOCK] = dr.ladder(1)[:dr.BLOCK]
    p[at[1] * dr.BLOCK:(at[1] + 1) * dr.BLOCK] = np.arange(dr.BLOCK) % 256
    p[at[2] * dr.BLOCK:(at[2] + 1) * dr.BLOCK] = np.random.default_rng(6).integers(0, 256, dr.BLOCK)
    return at


def _big_file(ctx, tmp_path, p, changed):
    bg = _background()
    (gz, gzi, payload), = _write(ctx, tmp_path, 8, [p], [(1, 0, None)])
    assert payload == p.tobytes()
    hists = {i: h for i, h in bg["hists"].items() if i not in changed}
    return _check(gz, gzi, payload, 1, code=False, hists=hists)


@pytest.fixture(scope="module")
def first_run(ctx, tmp_path_factory):
    bg = _background()
    assert len(bg["skip"]) == 88 and len(dr.unsampled(512)) == 0 and len(dr.unsampled(513)) == 1
    p = bg["payload"].copy()
    at = _special(p)
    return _big_file(ctx, tmp_path_factory.mktemp("deflate600"), p, at), at


def test_blocks_the_sample_skipped(first_run):
    """600 blocks, 512 sampled: three of the 88 others hold the ladder, every byte value and random bytes under a code built
    from ten literals — (a) to (f); the random block does not fit and is stored"""
    res, at = first_run
    assert len(res["sizes"]) == NBLOCKS and all(res["ll_lens"])
    assert res["stored"][at[2]]


def test_stored_block_threshold_to_the_byte(ctx, first_run, tmp_path):
    """sixteen unsampled blocks whose dynamic form takes 65503..65518 bytes under the file's code (found in a first run:
    unsampled blocks do not change it): up to 65510 bytes a dynamic block — BSIZE = 65535, the field's maximum, at 65510 —
    and a stored one from 65511"""
    first, special = first_run
    bg = _background()
    ll, dl, hb = first["ll_lens"], first["d_lens"], first["hdr_bits"]
    p = bg["payload"].copy()
    _special(p)
    sweep = bg["skip"][20:36]
    targets = list(range(65503, 65519))
    for b, t in zip(sweep, targets):
        blk = dr.fit_block(ll, dl, hb, t, t)
        assert dr.sbytes(dr.hist(blk, 1), ll, 1, dl, hb) == t
        p[b * dr.BLOCK:(b + 1) * dr.BLOCK] = blk
    assert {65509, 65510, 65511, 65512} <= set(targets)
    res = _big_file(ctx, tmp_path, p, set(sweep) | set(special))
    assert res["hdr_bits"] == hb and res["hdr"] == first["hdr"] and res["ll_lens"] == ll, "the sampled blocks are unchanged"
    for b, t in zip(sweep, targets):
        assert res["stored"][b] == (t > 65510), t
        assert res["sizes"][b] == (18 + t + 8 if t <= 65510 else 18 + 5 + dr.BLOCK + 8), t
    assert res["sizes"][sweep[targets.index(65510)]] == 65536
    assert res["sizes"][sweep[targets.index(65511)]] == 18 + 5 + dr.BLOCK + 8
