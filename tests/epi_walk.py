"""Which thread of the statistics pass meets which flush of the column sums' counter planes: a plain restatement of the WALK
of the kernels of panagram_amd/csrc/pg_rows.hip — no rows, no arithmetic, only the bookkeeping that decides when the planes
(pg_planes.h: eight planes, 255 rows) are emptied in the MIDDLE of a contig.  It restates
  the tiles of each contig (1024 rows; a contig's last one may be partial) and the bin length of include/panagram_hip.h;
  launch_rows_epilogue's grid — without the occupancy cap, which only bites beyond a thousand workgroups — and its test switch
  PG_EPI_WORKGROUPS (`bound`);
  epi_range: a workgroup's contiguous tiles, cut in units of 4 tiles (8 for one-byte rows);
  per tile the path the kernel takes — a group of full tiles of one contig (k_epilogue_n 4 tiles, k_epilogue_w PG_EPI_W_GQ12 /
  PG_EPI_W_GQ16 = 2), one windowed tile, one unwindowed tile — from binlen, epi_maxb_for, epi_minbin and the contig's end;
  `vrows`, the rows a thread has put into its planes: 4 per tile in k_epilogue_n / k_epilogue_w, 4 per iteration of 4 steps in
  k_epilogue_chunks (4 * IPT per full tile).
No tests in here: tests/test_rows_craft_cpu.py holds the cases of tests/test_gpu_planes_flush.py to the reach they claim.

Sites (Flush.site):
  n.group   k_epilogue_n<2..8>, group path: `if (vrows == PLANES_FLUSH) vflush();` inside rows16
  n.tile    k_epilogue_n<2..8>, one windowed tile: the same line at the end of the windowed branch
  w         k_epilogue_w<9..16>: `vrows + RPT > PLANES_CEIL` at the top of the tile loop, the contig unchanged
  chunks    k_epilogue_chunks: `if (vrows == PLANES_FLUSH) vflush();` after add4
  end       any of them: what the planes hold when the workgroup's range leaves the contig (or ends)"""
from collections import namedtuple

TILE = 1024
PLANES_CEIL, PLANES_FLUSH = 255, 240
EPI_MIN_TILES, MAX_GRID = 128, 2048
N_GROUP_TILES, W_GROUP_TILES = 4, 2

Flush = namedtuple("Flush", "site vrows contig tile wg")   # tile: the tile (a group's first) whose rows the thread had just taken
Walk = namedtuple("Walk", "flushes paths ranges")          # paths[tile] = "group" | "tile" | "unwindowed"; ranges[wg] = (begin, end)


def row_bytes(n):
    return (n + 7) // 8


def kernel_of(n):
    nb = row_bytes(n)
    return "b1" if nb == 1 else "n" if nb <= 8 else "w" if nb <= 16 else "chunks"


def maxb_for(n):
    return max(16, min(128, 3072 // (n + 1)))


def minbin(maxb):
    return (TILE + maxb - 3) // (maxb - 2)


def bin_length(nk, max_bin_len=200000, min_bin_count=100):
    binlen = max_bin_len
    if nk // binlen < min_bin_count:
        binlen = nk // min_bin_count
    return max(1, binlen)


def tiles_of(nks):
    """(tile_contig, tile0 per contig)"""
    tile_contig, tile0 = [], []
    for c, nk in enumerate(nks):
        tile0.append(len(tile_contig))
        tile_contig += [c] * ((nk + TILE - 1) // TILE)
    return tile_contig, tile0


def grid_for(ntiles, bound=None):
    grid = (ntiles + EPI_MIN_TILES - 1) // EPI_MIN_TILES
    grid = max(grid, min(1024, ntiles // 16))
    grid = max(1, min(MAX_GRID, grid))
    if bound is not None:
        grid = min(grid, max(1, min(MAX_GRID, bound)))
    return grid


def epi_range(gt, ntiles, j, n):
    ngroups = (ntiles + gt - 1) // gt
    return gt * (ngroups * j // n), min(ntiles, gt * (ngroups * (j + 1) // n))


def chunk_rows_per_tile(n, npos=TILE):
    """rows a lane of k_epilogue_chunks puts into its planes over a tile of npos rows"""
    c = (row_bytes(n) + 15) // 16
    iter_rows = 4 * (64 // c) * (TILE // 4 // 64)
    return 4 * sum(1 for r0 in range(0, TILE, iter_rows) if r0 < npos)


def walk(n, nks, bound=None, colsums=True, max_bin_len=200000, min_bin_count=100, **_):
    """the flushes of one launch over contigs of nks rows of n genomes, workgroup by workgroup"""
    kern = kernel_of(n)
    tile_contig, tile0 = tiles_of(nks)
    ntiles = len(tile_contig)
    binlen = [bin_length(nk, max_bin_len, min_bin_count) for nk in nks]
    maxb = maxb_for(n)
    grid = grid_for(ntiles, bound)
    gt = 8 if kern == "b1" else 4
    flushes, paths, ranges = [], {}, []
    for wg in range(grid):
        t_begin, t_end = epi_range(gt, ntiles, wg, grid)
        ranges.append((t_begin, t_end))
        if kern == "b1" or not colsums:  # (one-byte rows: accumulators of their own; no column sums: the planes stay empty)
            continue
        vrows, cur_c, tile, last = 0, None, t_begin, t_begin

        def leave():
            nonlocal vrows
            if cur_c is not None and vrows:
                flushes.append(Flush("end", vrows, cur_c, last, wg))
            vrows = 0

        while tile < t_end:
            c = tile_contig[tile]
            if kern == "w" and vrows and c == cur_c and vrows + 4 * W_GROUP_TILES > PLANES_CEIL:
                flushes.append(Flush("w", vrows, c, last, wg))
                vrows = 0
            if c != cur_c:
                leave()
                cur_c = c
            last = tile
            ts, bl, nk = (tile - tile0[c]) * TILE, binlen[c], nks[c]
            npos = min(TILE, nk - ts)
            if kern == "chunks":
                paths[tile] = "tile" if bl >= minbin(maxb) else "unwindowed"
                for _ in range(chunk_rows_per_tile(n, npos) // 4):
                    vrows += 4
                    if vrows == PLANES_FLUSH:
                        flushes.append(Flush("chunks", vrows, c, tile, wg))
                        vrows = 0
                tile += 1
                continue
            gq = N_GROUP_TILES if kern == "n" else W_GROUP_TILES
            span = gq * TILE
            nbg = (ts + span - 1) // bl - ts // bl + 1
            if (tile + gq - 1 < t_end and tile_contig[tile + gq - 1] == c and ts + span <= nk and
                    (nbg == 1 or (bl >= 4 * gq and nbg <= maxb))):
                for q in range(gq):
                    paths[tile + q] = "group"
                    vrows += 4
                    if kern == "n" and vrows == PLANES_FLUSH:
                        flushes.append(Flush("n.group", vrows, c, tile, wg))
                        vrows = 0
                tile += gq
                continue
            windowed = bl >= minbin(maxb)
            paths[tile] = "tile" if windowed else "unwindowed"
            if kern == "w" or windowed:  # (k_epilogue_n's unwindowed tile: one ballot per column, no planes)
                vrows += 4
                if kern == "n" and vrows == PLANES_FLUSH:
                    flushes.append(Flush("n.tile", vrows, c, tile, wg))
                    vrows = 0
            tile += 1
        leave()
    return Walk(flushes, paths, ranges)


def mid_contig(w, site, vrows=None):
    """{(wg, contig): the flushes at `site` (with `vrows` rows, if given) that one workgroup meets inside one contig AND that
    have rows of that contig behind the last of them — the workgroup's next flush is that contig's `end`}"""
    out = {}
    for i, f in enumerate(w.flushes):
        if f.site != site:
            continue
        out.setdefault((f.wg, f.contig), []).append((i, f))
    good = {}
    for key, fl in out.items():
        i = fl[-1][0]
        nxt = w.flushes[i + 1] if i + 1 < len(w.flushes) else None
        if nxt is not None and nxt.site == "end" and (nxt.wg, nxt.contig) == key:
            sel = [f for _, f in fl if vrows is None or f.vrows == vrows]
            if sel:
                good[key] = sel
    return good


def reaches(w, site, times=2, vrows=None):
    return any(len(fl) >= times for fl in mid_contig(w, site, vrows).values())


def find_bins(n, nks, bounds, want, candidates=range(8, 513)):
    """the shortest bins (max_bin_len = b, min_bin_count = 1: every contig of at least b rows gets bins of b rows) whose walk
    under one of `bounds` satisfies `want`, as a geometry for rows_craft.container; None if there is none"""
    for b in candidates:
        geom = dict(max_bin_len=b, min_bin_count=1)
        if any(want(walk(n, nks, bound, **geom)) for bound in bounds):
            return geom
    return None


def one_tile_bins(n, nks, bounds=(1,)):
    """k_epilogue_n's one-tile site: bins long enough for the window (MINBIN <= binlen) whose groups of 4 tiles are refused"""
    return find_bins(n, nks, bounds, lambda w: reaches(w, "n.tile"))


def carry_bins(n, nks, bounds=(1, 2)):
    """k_epilogue_w's flush at 252 rows (both carries held back): groups and single tiles in turn inside a contig, an odd
    number of single tiles between two flushes"""
    return find_bins(n, nks, bounds, lambda w: reaches(w, "w", times=1, vrows=252))
