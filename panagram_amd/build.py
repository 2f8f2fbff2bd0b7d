"""Build libpanagram_hip.so in-tree with hipcc for gfx950 (cross-compiles without a GPU).

The sources are compiled to objects IN PARALLEL and linked: pg_anchor.hip — 300 instantiations of k_probe / k_insert_tile, three
minutes of hipcc as one unit — goes in as three units (-DPG_ANCHOR_PART=0/1/2: the minimizer windows each unit instantiates; see
the top of that file), so a build takes about a minute of wall time on four cores.  UNITS is the tree's only list of them."""
from __future__ import annotations

import os
import shutil
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
LIB = os.path.join(HERE, "libpanagram_hip.so")
OBJ = os.path.join(HERE, "build")
SOURCES = ["pg_kernels.hip", "pg_anchor.hip", "pg_rows.hip", "pg_deflate.hip", "pg_inflate.hip", "pg_minhash.hip", "pg_bins.hip", "pg_pairs.hip", "pg_find.hip", "pg_patterns.hip", "pg_gaps.hip", "pg_profile.hip", "pg_knn.hip", "pg_tablestats.hip", "pg_synteny.hip", "pg_blocks.hip", "pg_variants.hip", "pg_copies.hip", "pg_genotype.hip", "pg_locate.hip", "pg_fastq.hip", "pg_place.hip", "pg_screen.hip", "pg_novel.hip", "pg_unitigs.hip", "pg_api.hip", "pg_api_kmc.hip", "pg_api_sketch.hip",
           "pg_api_seqset.hip", "pg_api_bgzf.hip", "pg_api_query.hip", "pg_api_patterns.hip", "pg_api_gaps.hip", "pg_api_profile.hip", "pg_api_tablestats.hip", "pg_api_synteny.hip", "pg_api_copies.hip", "pg_api_fastq.hip", "pg_api_screen.hip", "pg_api_novel.hip", "pg_bgzf.cpp"]
HEADERS = ["pg_device.h", "pg_kernels.h", "pg_planes.h", "pg_rowread.h", "pg_pairblocks.h", "pg_tablescan.h", "pg_guard.h", "pg_host.h", "pg_gaps_host.h", "pg_select_host.h", "pg_profile_host.h", "pg_blocks_link.h", "pg_blocks_host.h", "pg_blocks_pred.h", "pg_copies_host.h", "pg_genotype_host.h", "pg_keytable_dev.h", "pg_keytable_host.h", "pg_postable_dev.h", "pg_runscan.h", "pg_runs_host.h", os.path.join("..", "..", "include", "panagram_hip.h")]
# (source, extra defines, object name): the units of one build
UNITS = [("pg_anchor.hip", ["PG_ANCHOR_PART=2"], "pg_anchor_p2.o"), ("pg_anchor.hip", ["PG_ANCHOR_PART=1"], "pg_anchor_p1.o"),
         ("pg_anchor.hip", ["PG_ANCHOR_PART=0"], "pg_anchor_p0.o"), ("pg_rows.hip", [], "pg_rows.o"), ("pg_api.hip", [], "pg_api.o"),
         ("pg_api_bgzf.hip", [], "pg_api_bgzf.o"), ("pg_api_seqset.hip", [], "pg_api_seqset.o"), ("pg_api_sketch.hip", [], "pg_api_sketch.o"),
         ("pg_api_query.hip", [], "pg_api_query.o"), ("pg_api_patterns.hip", [], "pg_api_patterns.o"), ("pg_api_gaps.hip", [], "pg_api_gaps.o"),
         ("pg_api_profile.hip", [], "pg_api_profile.o"), ("pg_profile.hip", [], "pg_profile.o"),
         ("pg_api_kmc.hip", [], "pg_api_kmc.o"), ("pg_kernels.hip", [], "pg_kernels.o"),
         ("pg_deflate.hip", [], "pg_deflate.o"), ("pg_inflate.hip", [], "pg_inflate.o"), ("pg_minhash.hip", [], "pg_minhash.o"),
         ("pg_bins.hip", [], "pg_bins.o"), ("pg_pairs.hip", [], "pg_pairs.o"), ("pg_find.hip", [], "pg_find.o"), ("pg_patterns.hip", [], "pg_patterns.o"), ("pg_gaps.hip", [], "pg_gaps.o"),
         ("pg_knn.hip", [], "pg_knn.o"), ("pg_tablestats.hip", [], "pg_tablestats.o"), ("pg_api_tablestats.hip", [], "pg_api_tablestats.o"),
         ("pg_synteny.hip", [], "pg_synteny.o"), ("pg_blocks.hip", [], "pg_blocks.o"), ("pg_variants.hip", [], "pg_variants.o"),
         ("pg_api_synteny.hip", [], "pg_api_synteny.o"), ("pg_copies.hip", [], "pg_copies.o"), ("pg_genotype.hip", [], "pg_genotype.o"), ("pg_locate.hip", [], "pg_locate.o"), ("pg_api_copies.hip", [], "pg_api_copies.o"),
         ("pg_fastq.hip", [], "pg_fastq.o"), ("pg_place.hip", [], "pg_place.o"), ("pg_api_fastq.hip", [], "pg_api_fastq.o"),
         ("pg_screen.hip", [], "pg_screen.o"), ("pg_api_screen.hip", [], "pg_api_screen.o"),
         ("pg_novel.hip", [], "pg_novel.o"), ("pg_unitigs.hip", [], "pg_unitigs.o"), ("pg_api_novel.hip", [], "pg_api_novel.o"),
         ("pg_bgzf.cpp", [], "pg_bgzf.o")]
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-Wall", "-Wno-unused-function", "-Wno-unused-value", "-Wno-unused-result"]


def _stale() -> bool:
    if not os.path.exists(LIB):
        return True
    t = os.path.getmtime(LIB)
    return any(os.path.getmtime(os.path.join(CSRC, f)) > t for f in SOURCES + HEADERS)


def build(force: bool = False, verbose: bool = True, defines=(), out: str | None = None, csrc: str = CSRC, only=()) -> str:
    """Compile the HIP extension; returns the path of the shared library.
    ``defines`` (e.g. ["PG_PROBE_TILE=2048"]) override kernel tuning constants.
    A variant beside the product: ``out`` is the library to write (its objects go to build/<its name>/), ``csrc`` the source
    directory (another checkout's), ``only`` the sources that get the defines and are compiled — the objects of the others are
    those of the last plain build."""
    if not force and not defines and not out and not _stale():
        return LIB
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        raise RuntimeError("hipcc not found: cannot build libpanagram_hip.so")
    lib = os.path.abspath(out) if out else LIB
    objdir = os.path.join(OBJ, os.path.splitext(os.path.basename(lib))[0]) if out else OBJ
    os.makedirs(objdir, exist_ok=True)
    defines = list(defines)
    units = UNITS
    if any(d.split("=")[0] in ("PG_PHASE_TIMING", "PG_ANCHOR_PART") for d in defines) and (not only or "pg_anchor.hip" in only):
        units = [u for u in UNITS if u[0] != "pg_anchor.hip"] + [("pg_anchor.hip", [], "pg_anchor.o")]  # (one device variable / the caller's own split)

    def compile_unit(u):
        src, extra, obj = u
        if only and src not in only:
            return os.path.join(OBJ, obj)  # (of the last plain build)
        cmd = [hipcc] + FLAGS + ["-c", "-o", os.path.join(objdir, obj)] + [f"-D{d}" for d in defines + extra] + [os.path.join(csrc, src)]
        if verbose:
            print(" ".join(cmd), file=sys.stderr)
        subprocess.run(cmd, check=True)
        return os.path.join(objdir, obj)

    jobs = max(1, min(len(units), int(os.environ.get("PG_BUILD_JOBS", "0")) or (os.cpu_count() or 2)))
    with ThreadPoolExecutor(max_workers=jobs) as pool:
        objs = list(pool.map(compile_unit, units))
    cmd = [hipcc, "--offload-arch=gfx950", "-shared", "-fPIC", "-o", lib + ".tmp"] + objs + ["-lz", "-lpthread"]
    if verbose:
        print(" ".join(cmd), file=sys.stderr)
    subprocess.run(cmd, check=True)
    os.replace(lib + ".tmp", lib)
    return lib


if __name__ == "__main__":  # build.py [--force] [-DNAME=VALUE ...] [--out=LIB] [--csrc=DIR] [--only=a.hip,b.hip]
    opt = {a[2:].split("=", 1)[0]: a.split("=", 1)[1] for a in sys.argv[1:] if a.startswith("--") and "=" in a}
    build(force="--force" in sys.argv, defines=[a[2:] for a in sys.argv[1:] if a.startswith("-D")], out=opt.get("out"),
          csrc=opt.get("csrc", CSRC), only=[f for f in opt.get("only", "").split(",") if f])
